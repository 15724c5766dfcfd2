// voxel_sparse_host.hip -- pcp::VoxelDownSampleV3 / V2 on the device (voxel_sparse.hip): pcr_voxel_filter_sparse, pcr_voxel_sparse_order and the
// library-internal entry the whole-map call of submap.hip uses.

#include <algorithm>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace {

// the parameter that is out of range, named; nullptr when all are in range
const char* vs_params_out_of_range(double leaf, float gs, const pcr_voxel_sparse_params& p) {
    if (!(leaf > 0) || !(gs > 0.0f) || !std::isfinite(gs)) return "pcr_voxel_filter_sparse: leaf must be positive (and a positive finite float)";
    if (p.kind != PCR_VOXEL_SPARSE_V3 && p.kind != PCR_VOXEL_SPARSE_V2)
        return "pcr_voxel_filter_sparse: unknown kind (PCR_VOXEL_SPARSE_V3 = 3 or PCR_VOXEL_SPARSE_V2 = 2)";
    if (p.kind == PCR_VOXEL_SPARSE_V2 && p.max_voxel_pts < 1) return "pcr_voxel_filter_sparse: max_voxel_pts must be at least 1";
    if (p.kind == PCR_VOXEL_SPARSE_V2 && p.min_voxel_pts < 0) return "pcr_voxel_filter_sparse: min_voxel_pts must not be negative";
    return nullptr;
}

// Device memory in, device memory out: everything queued, then the call's one synchronisation.  *count = the voxels emitted (also beyond cap).
int vs_run(pcr_handle* h, const float* d_pts, size_t n, size_t sf, float gs, const pcr_voxel_sparse_params& p, float* d_out, size_t cap, size_t* count) {
    pcr_handle::Vs& v = h->vs;
    v.have_order = false;
    const VsSizes z = voxel_sparse_bytes(n);
    H_TRY(v.hdr.reserve(z.hdr));
    for (int i = 0; i < 2; ++i) { H_TRY(v.key[i].reserve(z.key)); H_TRY(v.row[i].reserve(z.row)); }
    H_TRY(v.hist.reserve(z.hist));
    H_TRY(v.cnt.reserve(z.cnt));
    H_TRY(v.first.reserve(z.first));
    H_TRY(v.lead.reserve(z.lead));
    H_TRY(v.tile.reserve(z.tile));
    H_TRY(v.ret.ensure());
    VsBuffers b;
    b.hdr = v.hdr.p;
    for (int i = 0; i < 2; ++i) { b.key[i] = v.key[i].as<unsigned long long>(); b.row[i] = v.row[i].as<uint32_t>(); }
    b.hist = v.hist.as<uint32_t>(); b.cnt = v.cnt.as<uint32_t>(); b.first = v.first.as<uint32_t>(); b.lead = v.lead.p; b.tile = v.tile.as<uint32_t>();
    H_TRY(voxel_sparse_launch(b, d_pts, sf, n, gs, p.kind, p.max_voxel_pts, p.min_voxel_pts, d_out, cap, v.ret.dev, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    const VsResult r = *v.ret.host;
    const std::string ext = std::to_string(r.ext[0]) + " x " + std::to_string(r.ext[1]) + " x " + std::to_string(r.ext[2]);
    if (r.refused == kVsRefusedRange)
        return fail(h, std::string("pcr_voxel_filter_sparse: ") + (p.kind == PCR_VOXEL_SPARSE_V3 ? "floor(p * inv)" : "p / gs") +
                           " leaves the int range on a row of the cloud (leaf " + std::to_string(gs) + "): refused");
    if (r.refused == kVsRefusedBits)
        return fail(h, "pcr_voxel_filter_sparse: the voxel key needs " + std::to_string(r.bits) + " bits, more than 64: extents " + ext +
                           " voxels (x, y, z): refused");
    v.have_order = true; v.order_n = r.kept; v.order_buf = r.passes & 1;
    *count = r.count;
    return 0;
}

}  // namespace

// (library-internal, for submap.hip: V3 of device memory into device memory; out_capacity >= n)
int pcr_internal_vs_v3(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity, size_t* n_out) {
    if (!h || !n_out) return 1;
    h->err.clear();
    *n_out = 0;
    if (!d_pts || !d_out || n == 0 || n > kMaxPoints || out_capacity < n) return fail(h, "sparse voxel filter: bad arguments");
    pcr_voxel_sparse_params p;
    pcr_voxel_sparse_default_params(&p);
    const float gs = (float)leaf;
    if (const char* bad = vs_params_out_of_range(leaf, gs, p)) return fail(h, bad);
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    return vs_run(h, static_cast<const float*>(d_pts), n, stride_bytes / 4, gs, p, static_cast<float*>(d_out), out_capacity, n_out);
}

extern "C" {

void pcr_voxel_sparse_default_params(pcr_voxel_sparse_params* p) {
    if (!p) return;
    p->kind = PCR_VOXEL_SPARSE_V3;
    p->max_voxel_pts = 20;      // VoxelDownSampleV2(float gs, int max_vp = 20, int min_vp = 0), pcp.hpp:100
    p->min_voxel_pts = 0;
}

int pcr_voxel_filter_sparse(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double leaf,
                            const pcr_voxel_sparse_params* params, void* out, size_t out_capacity, int out_on_device, size_t* n_out) {
    if (!h) return 1;
    h->err.clear();
    if (!n_out) return fail(h, "n_out is NULL");
    *n_out = 0;
    h->vs.have_order = false;
    if (n && !pts) return fail(h, "NULL cloud with nonzero size");
    if (out_capacity && !out) return fail(h, "NULL output with nonzero capacity");
    pcr_voxel_sparse_params p;
    pcr_voxel_sparse_default_params(&p);
    if (params) p = *params;
    const float gs = (float)leaf;      // the reference's `float gs`
    if (const char* bad = vs_params_out_of_range(leaf, gs, p)) return fail(h, bad);
    if (n > kMaxPoints) return fail(h, "cloud too large");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (n == 0) { h->vs.have_order = true; h->vs.order_n = 0; h->vs.order_buf = 0; return 0; }
    const float* d_pts = static_cast<const float*>(pts);
    if (!on_device && stage_host(h, &h->vs.in, pts, n, stride_bytes, &d_pts, true)) return 1;
    float* d_out = static_cast<float*>(out);
    size_t cap = out_capacity;
    if (!out_on_device) {
        cap = std::min(out_capacity, n);
        H_TRY(h->vs.out.reserve((cap ? cap : 1) * stride_bytes));
        d_out = h->vs.out.as<float>();
    }
    size_t count = 0;
    if (vs_run(h, d_pts, n, stride_bytes / 4, gs, p, d_out, cap, &count)) return 1;
    *n_out = count;
    if (count > out_capacity) return fail(h, "output capacity too small: " + std::to_string(count) + " voxels are emitted");
    if (!out_on_device && count) H_TRY(hipMemcpy(out, d_out, count * stride_bytes, hipMemcpyDeviceToHost));
    return 0;
}

int pcr_voxel_sparse_order(pcr_handle* h, uint64_t* keys, uint32_t* rows, size_t capacity, size_t* count) {
    if (!h) return 1;
    h->err.clear();
    if (!count) return fail(h, "count is NULL");
    *count = 0;
    if (!h->vs.have_order) return fail(h, "pcr_voxel_sparse_order: the last pcr_voxel_filter_sparse on this handle sorted nothing (none was made, or it was refused)");
    const size_t m = h->vs.order_n;
    *count = m;
    if ((keys || rows) && capacity < m) return fail(h, "pcr_voxel_sparse_order: capacity too small: " + std::to_string(m) + " rows were kept");
    if (m == 0 || set_device(h)) return m == 0 ? 0 : 1;
    const int b = h->vs.order_buf;
    if (keys) H_TRY(hipMemcpy(keys, h->vs.key[b].p, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rows) H_TRY(hipMemcpy(rows, h->vs.row[b].p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
