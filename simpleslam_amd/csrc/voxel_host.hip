// voxel_host.hip -- pcl::VoxelGrid on the device (voxel_filter.hip), queued and collected: pcr_voxel_filter and its two halves.

#include <algorithm>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace {

// The voxel filter in two halves: everything queued (vf_enqueue), then the one synchronisation and what its result asks for (vf_settle).
// pcr_voxel_filter is the two back to back; the sub-map assembly (submap.hip) queues an assembly with the first and collects it with the second when the
// sub-map is next asked for -- the kernels of an assembly then run beside the next scan's own filter (pcr_map_update_begin).
int vf_enqueue(pcr_handle* h) {
    const pcr_handle::Vf::Job& j = h->vf.job;
    if (h->vf.grid.build(j.d_pts, j.n, j.sf, j.leaf, h->stream, &h->err, 0.0, 1, nullptr, true) != hipSuccess) return 1;
    H_TRY(voxel_filter_launch(h->vf.grid, j.d_pts, j.sf, j.n, h->vf.head.as<uint32_t>(), h->vf.sums.as<uint32_t>(), h->vf.count.p, j.d_out, j.cap,
                              h->vf.ret, h->stream));
    return 0;
}
int vf_begin(pcr_handle* h, const float* d_pts, size_t n, size_t sf, double leaf, float* d_out, size_t cap) {
    // ONE round trip: the two launches of the filter are queued right behind the index build -- they read the header themselves and do nothing
    // when it says overflow, stale or empty -- and their last block writes the voxel count and the header's verdict into page-locked memory.
    // (Round 4 read the header first, then the count: two more synchronisations and an idle device in between, ~35 us of the 0.16 ms a
    //  65 536-point scan took: round 5, scripts/seq_breakdown.py.)
    // The index reuses the previous call's box and tile layout when the cloud still fits (GridIndex::hint_ok): the order of the voxels -- idx sorts by
    // (z, y, x) -- does not depend on where the box starts, so the output is the same either way; a cloud that does not fit comes back `stale` and is
    // built afresh, from then on with room around the box (a sub-map's box moves with the vehicle) and half as much again per bin.
    const size_t nr = std::max(n, h->vf.grid.reserve_points);
    H_TRY(h->vf.head.reserve((nr + 4096) * sizeof(uint32_t)));
    H_TRY(h->vf.sums.reserve((nr / 2048 + 2) * sizeof(uint32_t)));
    H_TRY(h->vf.count.reserve(voxel_filter_wave_bytes(nr)));
    if (!h->vf.ret) H_TRY(hipHostMalloc((void**)&h->vf.ret, sizeof(VfResult) + 64, hipHostMallocDefault));
    h->vf.grid.no_hints = h->prm.index_no_hints != 0;
    h->vf.grid.cut_sparse = true; h->vf.grid.coherent_input = true;
    // (room around the box and in the bins from the first build on: a handle's second cloud never fits the first one's tight box, and that build was made twice)
    if (h->vf.grid.hint_margin == 0) { h->vf.grid.hint_margin = 16; h->vf.grid.hint_margin_z_pcl = 4; h->vf.grid.lay_room_shift = 1; h->vf.grid.lay_room_add = 256; }
    h->vf.job = pcr_handle::Vf::Job{d_pts, n, sf, leaf, d_out, cap};
    return vf_enqueue(h);
}
int vf_settle(pcr_handle* h, uint32_t* count, int* too_fine) {
    volatile VfResult& ret = *reinterpret_cast<VfResult*>(h->vf.ret);
    for (int attempt = 0; attempt < 6; ++attempt) {
        if (attempt && vf_enqueue(h)) return 1;
        H_TRY(hipStreamSynchronize(h->stream));
        if (ret.stale) {      // the box (or a bin's room) taken over from the previous call does not hold this cloud
            // (the cell count the tile size goes by is kept once the box has its margin: a build without it takes the dense path -- 23 us instead of 11 for a scan)
            if (h->vf.grid.hint_margin == 0) { h->vf.grid.hint_margin = 16; h->vf.grid.hint_margin_z_pcl = 4; h->vf.grid.cells_hint = 0; }
            h->vf.grid.lay_room_shift = 1; h->vf.grid.lay_room_add = 256;
            continue;
        }
        if (!ret.overflow) {
            *count = ret.count; *too_fine = ret.too_fine;
            h->vf.grid.note_cells(ret.n_cells);
            if (!ret.empty && !ret.too_fine) h->vf.grid.confirm();
            return 0;
        }
        if (h->vf.grid.grow_cells(ret.n_cells, &h->err) != hipSuccess) return 1;
    }
    return fail(h, "voxel table could not be sized");
}

}  // namespace

// (library-internal, for submap.hip: a filter of device memory into device memory, queued / collected; out_capacity >= n)
int pcr_internal_vf_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity) {
    if (!h) return 1;
    h->err.clear();
    if (!d_pts || !d_out || n == 0 || n > kMaxPoints || out_capacity < n) return fail(h, "voxel filter: bad arguments");
    if (!(leaf > 0)) return fail(h, "leaf size must be positive");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    return vf_begin(h, static_cast<const float*>(d_pts), n, stride_bytes / 4, leaf, static_cast<float*>(d_out), out_capacity);
}
void pcr_internal_vf_reserve(pcr_handle* h, size_t points) { if (h && points <= kMaxPoints) h->vf.grid.reserve_points = std::max(h->vf.grid.reserve_points, points); }
int pcr_internal_vf_end(pcr_handle* h, size_t* n_out) {
    if (!h || !n_out) return 1;
    *n_out = 0;
    if (set_device(h)) return 1;
    uint32_t count = 0;
    int too_fine = 0;
    if (vf_settle(h, &count, &too_fine)) return 1;
    if (too_fine) {      // pcl::VoxelGrid: output = input (see pcr_voxel_filter)
        const pcr_handle::Vf::Job& j = h->vf.job;
        H_TRY(hipMemcpyAsync(j.d_out, j.d_pts, j.n * j.sf * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        *n_out = j.n;
        return 0;
    }
    *n_out = count;
    return 0;
}

extern "C" {

int pcr_voxel_filter(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double leaf, void* out,
                     size_t out_capacity, int out_on_device, size_t* n_out) {
    if (!h) return 1;
    h->err.clear();
    if (!n_out) return fail(h, "n_out is NULL");
    *n_out = 0;
    if (n && !pts) return fail(h, "NULL cloud with nonzero size");
    if (out_capacity && !out) return fail(h, "NULL output with nonzero capacity");
    if (!(leaf > 0)) return fail(h, "leaf size must be positive");
    if (n > kMaxPoints) return fail(h, "cloud too large");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (h->vf.inflight) return fail(h, "a voxel filter is queued on this handle (pcr_voxel_filter_begin): collect it with pcr_voxel_filter_end first");
    if (n == 0) return 0;
    const size_t sf = stride_bytes / 4;
    const float* d_pts = static_cast<const float*>(pts);
    if (!on_device && stage_host(h, &h->vf.in, pts, n, stride_bytes, &d_pts, true)) return 1;
    float* d_out = static_cast<float*>(out);
    size_t cap = out_capacity;
    if (!out_on_device) {
        cap = std::min(out_capacity, n);
        H_TRY(h->vf.out.reserve((cap ? cap : 1) * stride_bytes));
        d_out = h->vf.out.as<float>();
    }
    uint32_t count = 0;
    int too_fine = 0;
    if (vf_begin(h, d_pts, n, sf, leaf, d_out, cap) || vf_settle(h, &count, &too_fine)) return 1;
    if (too_fine) {
        // pcl::VoxelGrid: "Leaf size is too small for the input dataset. Integer indices would overflow." -> output = input
        *n_out = n;
        if (out_capacity < n) return fail(h, "output capacity too small (leaf too small for the data: the input is returned unfiltered)");
        H_TRY(hipMemcpyAsync(out, d_pts, n * stride_bytes, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        h->err = "leaf size too small for the input: integer voxel indices would overflow; input returned unfiltered";
        return 0;
    }
    *n_out = count;
    if (count > out_capacity) return fail(h, "output capacity too small: " + std::to_string(count) + " voxels are occupied");
    if (!out_on_device && count) H_TRY(hipMemcpy(out, d_out, (size_t)count * stride_bytes, hipMemcpyDeviceToHost));
    return 0;
}

int pcr_voxel_filter_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity) {
    if (!h) return 1;
    h->err.clear();
    if (h->vf.inflight) return fail(h, "a voxel filter is already queued on this handle: collect it with pcr_voxel_filter_end first");
    if (n && (!d_pts || !d_out)) return fail(h, "NULL cloud or output with nonzero size");
    if (out_capacity < n) return fail(h, "pcr_voxel_filter_begin needs room for n points (a leaf too small for the data returns the input unfiltered)");
    if (!(leaf > 0)) return fail(h, "leaf size must be positive");
    if (n > kMaxPoints) return fail(h, "cloud too large");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    h->vf.inflight_n = n;
    if (n && pcr_internal_vf_begin(h, d_pts, n, stride_bytes, leaf, d_out, out_capacity)) return 1;
    h->vf.inflight = true;
    return 0;
}

int pcr_voxel_filter_end(pcr_handle* h, size_t* n_out) {
    if (!h) return 1;
    if (!n_out) return fail(h, "n_out is NULL");
    *n_out = 0;
    if (!h->vf.inflight) return fail(h, "no voxel filter is queued on this handle");
    h->vf.inflight = false;
    h->err.clear();
    if (h->vf.inflight_n == 0) return 0;
    return pcr_internal_vf_end(h, n_out);
}

}  // extern "C"
