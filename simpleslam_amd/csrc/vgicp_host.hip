// vgicp_host.hip -- VGICP's host side: what is its own around PCL align() + LsqRegistration (lsq_registration_impl.hpp:53-171; the
// driver is lsq_host.h's run_lsq, GICP's too) -- a cut index's escapes, a region's repeat, the peer loop, the sharded fitness score --
// with the index levels of its covariance searches, the scan's side on its own stream, the region a target is prepared for
// (roi_enqueue: NDT uses it too), its row of the method table and the pcr_vgicp_* entry points.

#include <algorithm>

#include "lsq_host.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

int settle_grid(pcr_handle* h, GridIndex& g, const float* d_pts, size_t n, size_t stride_floats, double cell, int pcl_mode, const ClampBox* clamp) {
    for (int attempt = 0; attempt < 3; ++attempt) {
        if (g.build(d_pts, n, stride_floats, cell, h->stream, &h->err, 0.0, pcl_mode, clamp) != hipSuccess) return 1;
        GridHeader hdr;
        H_TRY(hipMemcpyAsync(&hdr, g.header.p, sizeof(hdr), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        if (!hdr.overflow) { g.note_cells(hdr.n_cells); return 0; }
        if (g.grow_cells(hdr.n_cells, &h->err) != hipSuccess) return 1;
    }
    return fail(h, "index could not be sized");
}

}  // namespace host
}  // namespace pcr

namespace {

// The coarse level pays for clouds with a long sparse tail -- raw or lightly filtered lidar scans, whose far points need
// dozens of rings on the fine grid -- and costs a little (another index build, de-duplication) on a voxel-filtered map of
// uniform density: measured 0.74 ms on one level vs 0.94 ms on three for the 1 M-point map, 7.7 ms vs 0.36 ms for the
// 65 k-point scan.  Scan-sized clouds get a second level, map-sized ones stay on one.  Two levels six cells apart (0.5 m and 3 m)
// beat the three levels four apart (0.5 / 2 / 8 m) this started with: the 8 m grid of a scan has a handful of cells holding most
// of its points -- three blocks sorted the whole scan, 120 us -- and each level is an index build on the side stream; A/B of the
// whole scan2map on one box: 3 x 4: 0.906 ms, 2 x 4: 0.917, 2 x 5: 0.890, 2 x 6: 0.875, 2 x 7: 0.900, 2 x 8: 0.880, 3 x 6: 0.975, 2 x 12: 1.25.
static constexpr double kCovRatio = 6.0;      // cell of a level / cell of the level below
static constexpr size_t kScanSizedMax = 300000;
bool scan_sized(size_t n) { return n <= kScanSizedMax; }
}  // namespace
namespace pcr {
namespace host {
int cov_levels(size_t n) { return scan_sized(n) ? 2 : 1; }
}  // namespace host
}  // namespace pcr
namespace {

int vgicp_side_init(pcr_handle* h) {
    if (!h->side_stream) {
        // The three streams of a VGICP call must be three HARDWARE queues.  The runtime spreads the streams of a process over a small pool
        // of queues per priority level (four by default), in the order they were created: in a process that had made a few streams
        // before -- bench.py's LOAM handles, any host application -- this handle's main and side stream came to share a queue, the scan's
        // side ran behind the target's kernels instead of beside them, and a call took 0.76 ms instead of 0.53.  Each priority level
        // has a pool of its own: the side stream asks for the highest, the auxiliary one for the lowest, the main one keeps the default.
        int prio_least = 0, prio_greatest = 0;
        H_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        H_TRY(hipStreamCreateWithPriority(&h->side_stream, hipStreamNonBlocking, prio_greatest));
        H_TRY(hipEventCreateWithFlags(&h->ev_side_in, hipEventDisableTiming));
        H_TRY(hipEventCreateWithFlags(&h->ev_side_done, hipEventDisableTiming));
        H_TRY(hipEventCreateWithFlags(&h->vg.ev_hdr, hipEventDisableTiming));
        H_TRY(hipEventCreateWithFlags(&h->vg.ev_aux_in, hipEventDisableTiming));
        H_TRY(hipEventCreateWithFlags(&h->vg.ev_aux_done, hipEventDisableTiming));
        H_TRY(hipStreamCreateWithPriority(&h->vg.aux_stream, hipStreamNonBlocking, prio_least));
        H_TRY(hipHostMalloc((void**)&h->side_hdr, 7 * sizeof(GridHeader), hipHostMallocDefault));
    }
    return 0;
}

// (inside settle_cov_levels: work may be in flight on the auxiliary stream -- never return before it has drained)
#define H_TRY_AUX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { if (aux) (void)hipStreamSynchronize(h->vg.aux_stream); return fail(h, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
}  // namespace
namespace pcr {
namespace host {
// the fine index plus the coarse ones of the covariance search, settled with one round trip
int settle_cov_levels(pcr_handle* h, GridIndex& g, GridIndex& l1, GridIndex& l2, const float* d_pts, size_t n, size_t stride_floats, double cell,
                      const CovSettle& opt) {
    const double shift0 = opt.shift0, ahead_cell = opt.ahead_cell;
    GridHeader* const hdr0_out = opt.hdr0_out;
    const bool may_cut = opt.may_cut, scan_levels = opt.scan_levels;
    bool *const ahead_ok = opt.ahead_ok, *const after_clean = opt.after_clean;
    const std::function<int()> *const after_ahead = opt.after_ahead, *const before_wait = opt.before_wait;
    BuildFilter* const filter0 = opt.filter0;
    GridIndex* lv[3] = {&g, &l1, &l2};
    const double cells[3] = {cell, kCovRatio * cell, kCovRatio * kCovRatio * cell};
    const int levels = cov_levels(n);
    bool todo[3] = {true, levels > 1, levels > 2};
    if (after_clean) *after_clean = false;
    if (after_ahead && vgicp_side_init(h)) return 1;
    int bulk_stage = 0;      // this call has cut the cloud to its bulk (1), to the room around one point (2)
    for (int attempt = 0; attempt < 5; ++attempt) {
        if (attempt > 0 && filter0) filter0->applied = filter0->tail_applied = false;      // (a repeat is a full build)
        GridHeader hdr_stack[4];
        GridHeader* hdr = after_ahead ? h->side_hdr + 3 : hdr_stack;      // (page-locked when the host is not to block in the copies)
        // (a one-level target's covariance grid at last call's cell size, enqueued with the fine level so that one round trip
        //  settles both; whether that size still suits the density is the caller's check)
        GridHeader& hdr_ahead = hdr[3];
        const bool ahead = ahead_cell > 0.0 && levels == 1 && attempt == 0 && !(h->clamp.use && may_cut);
        // ... on a stream of its own when the caller queues its work behind both (after_ahead): the two builds read the same cloud and
        // depend on nothing of each other, and neither fills the device (a chain of two or three launches of a few hundred blocks)
        const bool aux = ahead && after_ahead != nullptr && h->vg.aux_stream != nullptr;
        auto build_ahead = [&](hipStream_t s) -> int {
            l1.no_hints = h->prm.index_no_hints != 0;
            if (l1.build(d_pts, n, stride_floats, ahead_cell, s, &h->err, 0.0, 0, nullptr, true) != hipSuccess) return 1;
            H_TRY(hipMemcpyAsync(&hdr_ahead, l1.header.p, sizeof(GridHeader), hipMemcpyDeviceToHost, s));
            return 0;
        };
        if (aux) {
            H_TRY(hipEventRecord(h->vg.ev_aux_in, h->stream));      // (whatever brought the cloud here is on the main stream)
            H_TRY(hipStreamWaitEvent(h->vg.aux_stream, h->vg.ev_aux_in, 0));
            const int rc = build_ahead(h->vg.aux_stream);
            if (hipEventRecord(h->vg.ev_aux_done, h->vg.aux_stream) != hipSuccess || rc) { (void)hipStreamSynchronize(h->vg.aux_stream); return rc ? 1 : fail(h, "hipEventRecord failed"); }
        }
        for (int l = 0; l < 3; ++l) {
            if (!todo[l]) continue;
            // (the box and the tile layout of this index's previous build serve as hints -- GridIndex::hint_ok: a sub-map changes by a key frame
            //  at a time, a scan's box in the sensor frame hardly at all; a cloud that does not fit raises header.stale and is built afresh)
            lv[l]->no_hints = h->prm.index_no_hints != 0 || scan_levels;
            if (scan_levels) { lv[l]->prefer_one_level = true; lv[l]->header_mirror = nullptr; lv[l]->twin = nullptr; }
            if (lv[l]->build(d_pts, n, stride_floats, cells[l], h->stream, &h->err, l == 0 ? shift0 : 0.0, 0, h->clamp.use && may_cut ? &h->clamp : nullptr, !scan_levels,
                             l == 0 && attempt == 0 ? filter0 : nullptr) != hipSuccess) { if (aux) (void)hipStreamSynchronize(h->vg.aux_stream); return 1; }
            if (l == 0 && hdr0_out) H_TRY_AUX(lv[l]->enqueue_density(h->stream));
            H_TRY_AUX(hipMemcpyAsync(&hdr[l], lv[l]->header.p, sizeof(GridHeader), hipMemcpyDeviceToHost, h->stream));
        }
        if (aux) H_TRY_AUX(hipStreamWaitEvent(h->stream, h->vg.ev_aux_done, 0));
        else if (ahead && build_ahead(h->stream)) return 1;
        const bool early = ahead && after_ahead != nullptr;
        if (early) {
            H_TRY(hipEventRecord(h->vg.ev_hdr, h->stream));
            if ((*after_ahead)()) { (void)hipStreamSynchronize(h->stream); return 1; }
        }
        // (what the caller wants queued on OTHER streams while the host waits here: the scan's side of a scan2map call)
        if (before_wait && attempt == 0 && (*before_wait)()) { (void)hipStreamSynchronize(h->stream); return 1; }
        if (early) H_TRY(hipEventSynchronize(h->vg.ev_hdr));
        else H_TRY(hipStreamSynchronize(h->stream));
        if (ahead_ok) *ahead_ok = false;
        if (ahead && hdr_ahead.stale) { l1.hint_margin = 8; l1.cells_hint = 0; }      // (built afresh by the caller: it checks ahead_ok)
        else if (ahead && !hdr_ahead.overflow) { l1.note_cells(hdr_ahead.n_cells); if (!hdr_ahead.empty) l1.confirm(); if (ahead_ok) *ahead_ok = true; }
        bool again = false;
        for (int l = 0; l < 3; ++l) {
            if (!todo[l]) continue;
            if (hdr[l].stale) {      // the box (or a tile's room) taken over from the previous build does not hold this cloud: fresh box, padded from now on
                lv[l]->hint_margin = 8; lv[l]->cells_hint = 0;
                again = true;
                continue;
            }
            if (hdr[l].overflow) {
                if (hdr[l].n_cells > 4000000000ull && may_cut && (!h->clamp.use || bulk_stage == 1)) {
                    // a box no dense table can hold (a stray point far from the map): index the bulk of the cloud instead, all levels alike; when
                    // the index over the bulk box reports as much again (two sessions far apart), the room around one point of it
                    if (set_clamp_from_target_sample(h, bulk_stage == 1)) return 1;
                    bulk_stage += 1;
                    for (int k = 0; k < 3; ++k) todo[k] = k < levels;
                    again = true;
                    break;
                }
                if (hdr[l].n_cells > 4000000000ull && opt.untabulatable) *opt.untabulatable = true;      // (grow_cells refuses it)
                if (lv[l]->grow_cells(hdr[l].n_cells, &h->err) != hipSuccess) return 1;
                again = true;
            }
            else { todo[l] = false; lv[l]->note_cells(hdr[l].n_cells); if (!hdr[l].empty && !h->clamp.use) lv[l]->confirm(); if (l == 0 && hdr0_out) *hdr0_out = hdr[0]; }
        }
        if (!again) { if (after_clean) *after_clean = early && !hdr_ahead.stale && !hdr_ahead.overflow; return 0; }
    }
    return fail(h, "index could not be sized");
}
}  // namespace host
}  // namespace pcr
namespace {
// ... of a scan that did not come through vgicp_source_enqueue (pcr_vgicp_covariances, the redo of vgicp_source_settle): its levels, the checked way
int settle_scan_levels(pcr_handle* h, const float* d_pts, size_t n, size_t stride_floats) {
    CovSettle opt;
    opt.scan_levels = true;
    return settle_cov_levels(h, h->src_grid, h->vg.src_l1, h->vg.src_l2, d_pts, n, stride_floats, h->prm.vgicp_resolution, opt);
}

}  // namespace

namespace pcr {
namespace host {

// Source side of a VGICP scan2map call (its own index levels + covariances, fast_gicp_impl.hpp:103-108) enqueued on the side
// stream BEFORE the target is prepared on the main one: the 65 k-point covariance search is latency-bound and hides under
// the target's kernels.  Speculative about the cell tables: an overflowing level makes its kernels return early, which
// vgicp_source_settle() detects from the headers and redoes in order.
// The point of the main stream the scan's side may start behind (its staging copy, if any, is on the main stream): recorded BEFORE the
// target's work is queued there, so that a source side enqueued later (vgicp_source_enqueue(.., marked)) does not wait for that work.
int vgicp_source_mark(pcr_handle* h) {
    if (vgicp_side_init(h)) return 1;
    H_TRY(hipEventRecord(h->ev_side_in, h->stream));
    return 0;
}
// errp: where messages go (the worker thread's own string while the calling thread may be writing h->err)
int vgicp_source_enqueue(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, bool marked, std::string* errp) {
    std::string& err = errp ? *errp : h->err;
#define S_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(_e); return 1; } } while (0)
    h->side_pending = false;
    if (!marked && vgicp_side_init(h)) return 1;      // (marked: vgicp_source_mark has made the streams and events)
    if (n_src > kMaxPoints) return 0;                         // run_vgicp reports it
    S_TRY(h->vg.src_cov6.reserve((n_src + 1) * 6 * sizeof(double)));
    if (!marked) S_TRY(hipEventRecord(h->ev_side_in, h->stream));             // the scan's staging copy (if any) is on the main stream
    S_TRY(hipStreamWaitEvent(h->side_stream, h->ev_side_in, 0));
#undef S_TRY
    GridIndex* lv[3] = {&h->src_grid, &h->vg.src_l1, &h->vg.src_l2};
    const double cell = h->prm.vgicp_resolution, cells[3] = {cell, kCovRatio * cell, kCovRatio * kCovRatio * cell};
    const int levels = cov_levels(n_src);
    // from here on kernels reading the caller's d_src may be queued on the side stream: an error must not return before they
    // have drained (the caller is free to release d_src as soon as the call has failed)
    hipError_t e = hipSuccess;
    for (int l = 0; l < levels && e == hipSuccess; ++l) {
        // (no hints here: the box and the tile layout of one scan do not hold the next -- walls at other distances, other tiles crowded;
        //  measured: every call's hint failed and the redo cost 0.9 ms)
        // (a scan's points crowd around the sensor: on the coarse level a few cells hold a third of the scan, and the tiled build leaves
        //  them to ONE block, 94-146 us in the trace; on the fine level the crowded tiles still cost 34 us where the one-level build
        //  -- histogram with ranks, scan of the table, scatter -- takes ~30 us for the whole level.  A/B: 0.571 -> 0.54 ms per scan)
        lv[l]->prefer_one_level = true;
        // (one pass over the scan finds the box of both levels, and the headers go to the host from the kernel that makes them: a build
        //  without hints changes nothing in its header afterwards)
        lv[l]->header_mirror = &h->side_hdr[l];
        lv[l]->twin = (l == 0 && levels > 1) ? lv[1] : nullptr;
        lv[l]->twin_cell = cells[1];
        e = lv[l]->build(d_src, n_src, stride_floats, cells[l], h->side_stream, &err, 0.0);
        lv[l]->twin = nullptr;
        if (e == hipSuccess && !lv[l]->mirrored && (e = hipMemcpyAsync(&h->side_hdr[l], lv[l]->header.p, sizeof(GridHeader), hipMemcpyDeviceToHost, h->side_stream)) != hipSuccess)
            err = std::string("hipMemcpyAsync(side header): ") + hipGetErrorString(e);
    }
    if (e == hipSuccess && (e = vgicp_launch_cov(h->src_grid, levels > 1 ? &h->vg.src_l1 : nullptr, levels > 2 ? &h->vg.src_l2 : nullptr, d_src, stride_floats, n_src,
                                                 h->vg.src_cov6.as<double>(), h->side_stream, h->prm.vgicp_regularization, nullptr, nullptr, &h->vg.src_scratch,
                                                 (h->profile >= 2 && h->ev_cov[2] && n_src > 0 && scan_sized(n_src)) ? h->ev_cov + 2 : nullptr)) != hipSuccess)
        err = std::string("vgicp_launch_cov: ") + hipGetErrorString(e);
    if (e == hipSuccess && h->profile >= 2 && h->ev_cov[2] && n_src > 0 && scan_sized(n_src)) h->ev_cov_src_used = true;
    h->fit_copied_from = nullptr;
    if (e == hipSuccess && !sharded(h) && n_src > 0) {      // the scan, kept for a later pcr_fitness() (off the critical path here)
        const size_t bytes = n_src * stride_floats * sizeof(float);
        if ((e = h->fit_src.reserve(bytes)) != hipSuccess || (e = hipMemcpyAsync(h->fit_src.p, d_src, bytes, hipMemcpyDeviceToDevice, h->side_stream)) != hipSuccess)
            err = std::string("keeping the scan for the fitness score: ") + hipGetErrorString(e);
        else h->fit_copied_from = d_src;
    }
    if (e == hipSuccess && (e = hipEventRecord(h->ev_side_done, h->side_stream)) != hipSuccess) err = std::string("hipEventRecord: ") + hipGetErrorString(e);
    if (e != hipSuccess) { (void)hipStreamSynchronize(h->side_stream); return 1; }
    h->side_pending = true; h->side_src = d_src; h->side_n = n_src; h->side_stride = stride_floats;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace pcr {
namespace host {

// Source covariances ready on return (ordered before whatever the main stream runs next).
int vgicp_source_settle(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats) {
    const int levels = cov_levels(n_src);
    if (h->side_pending && h->side_src == d_src && h->side_n == n_src && h->side_stride == stride_floats) {
        h->side_pending = false;
        H_TRY(hipEventSynchronize(h->ev_side_done));
        bool overflow = false;
        GridIndex* lv[3] = {&h->src_grid, &h->vg.src_l1, &h->vg.src_l2};
        for (int l = 0; l < levels; ++l) {
            overflow = overflow || h->side_hdr[l].overflow != 0 || h->side_hdr[l].stale != 0;
            if (h->side_hdr[l].stale) { lv[l]->hint_margin = 8; lv[l]->cells_hint = 0; }      // (redone below, with a fresh box)
        }
        if (!overflow) {
            for (int l = 0; l < levels; ++l) { lv[l]->note_cells(h->side_hdr[l].n_cells); if (!h->side_hdr[l].empty) lv[l]->confirm(); }
            H_TRY(hipStreamWaitEvent(h->stream, h->ev_side_done, 0));
            return 0;
        }
    } else {
        H_TRY(side_drain(h));             // never leave side work in flight behind the caller's back
    }
    if (settle_scan_levels(h, d_src, n_src, stride_floats)) return 1;
    H_TRY(h->vg.src_cov6.reserve((n_src + 1) * 6 * sizeof(double)));
    H_TRY(vgicp_launch_cov(h->src_grid, levels > 1 ? &h->vg.src_l1 : nullptr, levels > 2 ? &h->vg.src_l2 : nullptr, d_src, stride_floats, n_src,
                           h->vg.src_cov6.as<double>(), h->stream, h->prm.vgicp_regularization, nullptr, nullptr, &h->vg.src_scratch));
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace pcr {
namespace host {

// Marks the macro cells of h->grid's lattice that `scan` can reach from its initial pose and fills `view`: base_m metres in any direction
// plus kRoiPerMetre metres per metre of distance from the sensor (a rotation of 0.05 rad = 2.9 degrees moves a point 100 m away by 5 m).
// The pose goes through a Matrix4f first, as VGICP and NDT hand their guess over as one.
static constexpr double kRoiPerMetre = 0.05;
int roi_enqueue(pcr_handle* h, const RoiScan& scan, double cell, double base_m, RoiView* view) {
    int ms = 0;      // macro cell of about 2 m
    while (ms < 5 && cell * (double)(1 << ms) < 2.0 * (1.0 - 1e-9)) ++ms;
    h->roi.mshift = ms;
    const size_t bytes = h->grid.cell_capacity + 4096;      // macro cells <= cells <= capacity (a build that needs more raises header.overflow)
    for (DeviceBuf* b : {&h->roi.mark[0], &h->roi.mark[1]}) {
        const void* before = b->p;
        H_TRY(b->reserve(bytes));
        if (b->p != before) H_TRY(hipMemsetAsync(b->p, 0, b->cap, h->stream));      // the marks start out clear; every call clears the other buffer for the next
    }
    // Every call clears the OTHER mark buffer for the next one -- over the macro cells of ITS lattice only.  When the lattice changes
    // (another box, another cell count) marks of the old one would survive beyond the new one's extent as spurious region: harmless for the
    // result (the mask only grows), wasteful.  An asynchronous memset then.
    if (h->roi.cells_seen != h->grid.cells_hint) {
        for (DeviceBuf* b : {&h->roi.mark[0], &h->roi.mark[1]}) H_TRY(hipMemsetAsync(b->p, 0, b->cap, h->stream));
        h->roi.cells_seen = h->grid.cells_hint;
    }
    for (DeviceBuf* b : {&h->roi.tmp, &h->roi.mask}) H_TRY(b->reserve(bytes));      // (written in full by every call)
    H_TRY(h->roi.esc.reserve(64));
    Pose16 T;
    for (int i = 0; i < 16; ++i) T.m[i] = (double)(float)scan.pose[i];
    const int k = h->roi.idx;
    const bool rider = h->blob_pending;
    if (rider) h->blob.zero = h->roi.esc.as<uint32_t>();      // (the escape counter starts at zero with the state)
    H_TRY(roi_launch(h->grid, scan.d_src, scan.n_src, scan.stride_floats, T, ms, h->roi.mark[k].as<uint8_t>(), h->roi.mark[k ^ 1].as<uint8_t>(),
                     h->roi.tmp.as<uint8_t>(), h->roi.mask.as<uint8_t>(), base_m, kRoiPerMetre, h->stream, rider ? &h->blob : nullptr));
    if (rider) { h->blob_pending = false; h->blob_stored = true; }
    h->roi.idx ^= 1;
    view->lat = h->grid.header.as<GridHeader>(); view->mask = h->roi.mask.as<uint8_t>(); view->escapes = h->roi.esc.as<uint32_t>();
    view->mshift = ms; view->filtered = 0; view->count = prof_counters(h);
    return 0;
}
RoiView roi_view(const pcr_handle* h) {      // the region the handle's target was prepared for (the mask of the LAST roi_enqueue)
    RoiView v;
    memset(&v, 0, sizeof v);
    if (h->roi_on) { v.lat = h->grid.header.as<GridHeader>(); v.mask = h->roi.mask.as<uint8_t>(); v.escapes = h->roi.esc.as<uint32_t>(); v.mshift = h->roi.mshift; }
    return v;
}

// The base margin, in metres, of the region a VGICP target is prepared for: 1 m of translation, plus the voxel that DIRECT7 / DIRECT27 reach beyond
// the cell a point lands in (pcr_params.vgicp_search).  The region is a dilation by a Chebyshev radius -- a box, not a ball (grid_index.hip) -- so
// the one voxel per axis that holds DIRECT7's face cells holds DIRECT27's edge and corner cells as well.  DIRECT1 keeps what it had.
static double vgicp_roi_margin(int search, double res) { return search == PCR_VGICP_DIRECT1 ? 1.0 : 1.0 + res; }

// keep_clamp: the caller has set h->clamp (a region cut around a scan, vgicp_align_recut): index that region instead of deciding here
int vgicp_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, const RoiScan* roi_scan, bool keep_clamp,
                         const std::function<int()>* before_wait) {
    h->target_ready = false;
    h->roi_on = false;
    const double res = h->prm.vgicp_resolution;
    if (!(res > 0)) return fail(h, "vgicp_resolution must be positive");
    if (h->prm.vgicp_k_corr != 20) return fail(h, "this build supports vgicp_k_corr = 20 (the reference's value) only");
    if (!keep_clamp) h->clamp.use = 0;
    h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats;
    bool ahead_ok = false;
    const double ahead_cell = (cov_levels(n_dst) == 1 && h->cov_scale_hint >= 1.3) ? res * h->cov_scale_hint : 0.0;
    CovCheck chk;
    const bool check = h->use_tile && h->have_halo;
    // prepared for one scan: covariances and voxels only where that scan can land (a cut index keeps the full preparation: its
    // escape accounting is of another kind)
    RoiView roi;
    memset(&roi, 0, sizeof roi);
    const bool want_roi = roi_scan && roi_scan->n_src > 0 && n_dst > 0 && !check;
    // region, covariances and voxels over (lattice, search grid): enqueued by settle_cov_levels behind the grid it builds ahead, before the
    // host has seen a header (the device used to idle ~45 us between the header read-back and the first of these launches), or below
    // ... and, from a handle's second call on, the voxel LATTICE holds the region's points only (BuildFilter, as NDT's: the region is marked first, on
    // the lattice of the previous full build, and the bin pass drops every point outside it -- a tenth of the map's points go through the two passes and
    // the voxel kernel; A/B on one box, round 5: preparation 0.372 -> 0.344 ms).  Needs the covariance search on a grid of its own (the grid built
    // ahead: it holds every point, and serves the fitness score), the previous full build's header and tile layout as hints (build() checks), and
    // lookups that test the mask first (vgicp.hip: vgicp_lookup, RoiView::filtered).
    BuildFilter bf;
    bf.enqueue_mask = [&]() -> hipError_t {
        if (roi_enqueue(h, *roi_scan, res, vgicp_roi_margin(h->prm.vgicp_search, res), &roi)) return hipErrorUnknown;      // 1 m of translation (+ the neighbourhood's voxel) + 0.05 rad
        bf.mask = roi.mask; bf.mshift = roi.mshift;
        return hipSuccess;
    };
    auto enqueue_rest = [&](const GridIndex* cov_grid) -> int {
        h->roi_on = false;
        if (bf.applied && !h->clamp.use) {      // (the region was marked inside the lattice's build)
            roi.filtered = 1;
            h->roi_on = true;
        } else if (want_roi && !h->clamp.use) {
            if (roi_enqueue(h, *roi_scan, res, vgicp_roi_margin(h->prm.vgicp_search, res), &roi)) return 1;      // 1 m of translation (+ the neighbourhood's voxel) + 0.05 rad
            h->roi_on = true;
        }
        H_TRY(vgicp_launch_cov(*cov_grid, cov_levels(n_dst) > 1 ? &h->cov_l1 : nullptr, cov_levels(n_dst) > 2 ? &h->vg.cov_l2 : nullptr, d_dst, stride_floats,
                               n_dst, h->vg.tgt_cov6.as<double>(), h->stream, h->prm.vgicp_regularization, check ? &chk : nullptr, h->roi_on ? &roi : nullptr,
                               &h->vg.tgt_scratch, (h->profile >= 2 && h->ev_cov[0] && !scan_sized(n_dst)) ? h->ev_cov : nullptr));
        if (h->profile >= 2 && h->ev_cov[0] && !scan_sized(n_dst)) h->ev_cov_tgt_used = true;
        H_TRY(vgicp_launch_voxels(h->grid, h->vg.tgt_cov6.as<double>(), h->vg.vox.as<VgicpVoxel>(), h->stream, h->prm.vgicp_regularization, h->prm.vgicp_voxel_mode,
                                  h->roi_on ? &roi : nullptr));
        return 0;
    };
    H_TRY(h->vg.tgt_cov6.reserve((n_dst + 1) * 6 * sizeof(double)));
    H_TRY(h->vg.vox.reserve((n_dst + 1) * sizeof(VgicpVoxel)));
    const std::function<int()> early = [&]() -> int { return enqueue_rest(&h->cov_l1); };
    bool early_clean = false;
    const bool try_early = want_roi && ahead_cell > 0.0 && !h->clamp.use;
    // (may_cut: a cloud too spread out for dense tables -- a stray point kilometres off -- is indexed over its bulk.  A rank of a sharded call
    //  too: its cloud is its own, the cut is its own decision, and a scan that reaches the cut fails the call on EVERY rank, run_vgicp)
    const bool try_filter = try_early && h->prm.index_no_hints == 0;
    CovSettle opt;
    opt.shift0 = 0.5; opt.hdr0_out = &h->vg.cov_hdr0; opt.may_cut = true; opt.ahead_cell = ahead_cell; opt.ahead_ok = &ahead_ok;
    opt.after_ahead = try_early ? &early : nullptr; opt.after_clean = &early_clean; opt.before_wait = before_wait;
    opt.filter0 = try_filter ? &bf : nullptr;
    if (settle_cov_levels(h, h->grid, h->cov_l1, h->vg.cov_l2, d_dst, n_dst, stride_floats, res, opt)) return 1;
    if (h->clamp.use) { ahead_ok = false; early_clean = false; }      // (the target was cut to its bulk in there: the grid built ahead covers the uncut cloud)
    h->have_target = true;
    // (a map-sized cloud is searched on ONE level of a cell of its own: cov_search_scale)
    const GridIndex* cov_grid = &h->grid;
    bool kept_ahead = false;
    if (bf.applied) {      // (the density figure of a region-only lattice is the region's: the search cell of the previous call stays -- it decides how many candidates a search visits, never its result)
        if (!ahead_ok && settle_grid(h, h->cov_l1, d_dst, n_dst, stride_floats, res * h->cov_scale_hint, 0, nullptr)) return 1;      // (the grid built ahead did not stand: built again, in full)
        kept_ahead = ahead_ok; cov_grid = &h->cov_l1;
    } else if (const double scale = cov_search_scale(h->vg.cov_hdr0, n_dst); scale > 0.0) {
        // the grid built ahead serves if its cell is within 15 % of what this cloud's density asks for (the cell only decides how
        // many candidates a search visits, never its result)
        const bool keep = ahead_ok && fabs(h->cov_scale_hint / scale - 1.0) <= 0.15;
        if (!keep) {
            if (settle_grid(h, h->cov_l1, d_dst, n_dst, stride_floats, res * scale, 0, h->clamp.use ? &h->clamp : nullptr)) return 1;
            h->cov_scale_hint = scale;
        }
        kept_ahead = keep;
        cov_grid = &h->cov_l1;
    } else h->cov_scale_hint = 0.0;
    if (check) {
        // sharded target (pcr_set_shard): the covariances of the points that can enter a voxel of the tile must be the whole
        // map's -- every neighbourhood of a point within one voxel of the tile has to end inside the halo
        H_TRY(h->vg.cov_viol.reserve(16));
        H_TRY(hipMemsetAsync(h->vg.cov_viol.p, 0, 16, h->stream));
        shard_extent(h, chk.ext_lo, chk.ext_hi);
        for (int d = 0; d < 3; ++d) { chk.chk_lo[d] = h->tile_lo[d] - res; chk.chk_hi[d] = h->tile_hi[d] + res; }
        chk.violations = h->vg.cov_viol.as<uint32_t>();
    }
    if (!(early_clean && kept_ahead) && enqueue_rest(cov_grid)) return 1;
    if (check) {
        uint32_t viol = 0;
        H_TRY(hipMemcpyAsync(&viol, h->vg.cov_viol.p, sizeof viol, hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        if (viol) return fail(h, std::to_string(viol) + " target points near this rank's tile have their 20 nearest neighbours reaching past the halo of " +
                                 std::to_string(h->halo) + " m: shard the map with a wider halo");
    }
    h->target_ready = true;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

// entries of the table of a pcr_params.vgicp_search (rows of slots in VgicpArgs::corr_slot)
size_t vgicp_table_entries(int search) { return search == PCR_VGICP_DIRECT27 ? 27 : search == PCR_VGICP_DIRECT7 ? 7 : 1; }

// The arguments of the handle's VGICP launches over a source (run_vgicp, pcr_vgicp_linearize): the whole target prepared, the index not cut
VgicpArgs vgicp_args(const pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats) {
    VgicpArgs a;
    memset(&a, 0, sizeof a);      // (roi.mask = nullptr, escapes = nullptr)
    a.src = d_src; a.n_src = (uint32_t)n_src; a.src_stride = (uint32_t)stride_floats;
    a.src_cov6 = h->vg.src_cov6.as<double>();
    a.hdr = h->grid.header.as<GridHeader>();
    a.cell_start = h->grid.cell_start.as<uint32_t>();
    a.vox = h->vg.vox.as<VgicpVoxel>();
    a.corr_slot = h->vg.corr_slot.as<uint32_t>(); a.corr_M = h->vg.corr_M.as<double>();
    a.corr_slot_next = h->vg.corr_slot2.as<uint32_t>(); a.corr_M_next = h->vg.corr_M2.as<double>();
    a.corr_T = h->vg.corr_T.as<double>(); a.corr_T_next = h->vg.corr_T2.as<double>();
    a.partials = h->vg_partials.as<double>();
    a.use_tile = h->use_tile;
    a.search = h->prm.vgicp_search;
    for (int d = 0; d < 3; ++d) { a.tile_lo[d] = h->tile_lo[d]; a.tile_hi[d] = h->tile_hi[d]; }
    return a;
}

int run_vgicp(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) {
    if (!h->target_ready) return fail(h, "no target prepared");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    if (ensure_out32(h)) return 1;
    const bool kept = fitness_scan_kept(h, d_src);
    // source covariances over the source's own index (fast_gicp_impl.hpp:103-108): already in flight when this is a
    // scan2map call, computed here otherwise
    if (vgicp_source_settle(h, d_src, n_src, stride_floats)) return 1;
    if (keep_scan_for_fitness(h, d_src, n_src, stride_floats, kept)) return 1;
    // the correspondence buffers, by the neighbourhood in force (VgicpArgs): DIRECT1 a slot and an M per point; DIRECT7 / DIRECT27 K + 1 rows of slots and
    // the linearisation's pose
    h->vg.lin_valid = false;
    const int search = h->prm.vgicp_search;
    if (sharded(h) && search != PCR_VGICP_DIRECT1) return fail(h, "internal: vgicp_search beyond DIRECT1 on a sharded handle");
    const size_t slot_rows = search == PCR_VGICP_DIRECT1 ? 1 : vgicp_table_entries(search) + 1;
    H_TRY(h->vg.corr_slot.reserve((n_src + 1) * slot_rows * sizeof(uint32_t)));
    H_TRY(h->vg.corr_slot2.reserve((n_src + 1) * slot_rows * sizeof(uint32_t)));
    if (search == PCR_VGICP_DIRECT1) {
        H_TRY(h->vg.corr_M.reserve((n_src + 1) * 6 * sizeof(double)));
        H_TRY(h->vg.corr_M2.reserve((n_src + 1) * 6 * sizeof(double)));
    } else {
        H_TRY(h->vg.corr_T.reserve(16 * sizeof(double)));
        H_TRY(h->vg.corr_T2.reserve(16 * sizeof(double)));
    }
    VgicpArgs a = vgicp_args(h, d_src, n_src, stride_floats);
    a.roi = roi_view(h);
    if (h->clamp.use) {      // the target index was cut to the bulk of the cloud (vgicp_prepare_target): watch where the scan goes
        H_TRY(h->vg.cov_viol.reserve(16));
        H_TRY(hipMemsetAsync(h->vg.cov_viol.p, 0, 16, h->stream));
        a.escapes = h->vg.cov_viol.as<uint32_t>() + 1;
        a.guard_cells = (int)ceil(std::max(4.0, 8.0 * h->prm.vgicp_resolution) / h->prm.vgicp_resolution);      // the reach of a 20-neighbour covariance (as pcr_set_shard's halo)
        if (search != PCR_VGICP_DIRECT1) a.guard_cells += 1;      // ... around every voxel a point is paired with: one voxel beyond its own
    }
    const bool shard = sharded(h);      // every rank linearises its tile's share of the scan; H, b and the error are summed over the ranks

    // ---- the device-resident loop of lsq_host.h's run_lsq.  Not for sharded targets (every pass's sums cross the ranks) and not when
    // pcr_params.host_optimiser asks for the host loop ----
    // Sharded over the peer exchange (pcr_comm_init_peer) the loop stays on the device too: an exchange launch in front of every pass
    // (vgicp.hip: vgicp_peer_exchange_kernel), and the host queues launches by a rule that gives every rank the same number of them (PaceRule).
    const bool peer_loop = shard && h->comm.peer_on && !h->comm.host_ar && !h->comm.rccl;
    const bool on_device = n_src > 0 && (!shard || peer_loop) && h->prm.host_optimiser == 0 && h->prm.vgicp_max_iters > 0;
    if (h->roi_on && !on_device) return fail(h, "internal: a target prepared for one scan needs the device-resident loop");
    if (peer_loop && peer_check(h)) return 1;
    if (on_device) {
        H_TRY(h->vg_partials.reserve((size_t)2 * 512 * 32 * sizeof(double)));
        a.partials = h->vg_partials.as<double>();
        if (peer_loop) H_TRY(h->vg.reduced.reserve(64 * sizeof(double)));
    }
    auto device_pass = [&](long i, VgCtl* d_ctl, VgOut* d_out, double seq) -> hipError_t {
        if (!peer_loop) return vgicp_launch_pass_pro(a, d_ctl, h->vg_partials.as<double>(), d_out, h->stream, seq, (int)i);
        if (i > 0) h->comm.peer_seq += 1.0;      // (the first launch of a call has nothing to exchange)
        return vgicp_launch_pass_pro(a, d_ctl, h->vg_partials.as<double>(), d_out, h->stream, seq, (int)i, &h->comm.peer, h->comm.peer_seq, h->vg.reduced.as<double>());
    };
    // ---- its host-driven loop; sharded, every pass's sums cross the ranks.  The LM trial pass (vgicp_launch_error) also linearises at the
    // trial pose: once a trial is accepted that pose IS the next linearisation point, so its H, b, error and correspondences are already
    // there (same values as a separate linearize() would return) and the state's parity says which of the two correspondence buffers
    // they are in ----
    auto host_pass = [&](int kind, int parity, const Pose16& xi, double seq) {
        return (kind == kVgPassLinearize ? vgicp_launch_linearize : vgicp_launch_error)(swapped(a, parity), xi, h->out32.dev, h->stream, seq);
    };
    LsqResult r;
    if (run_lsq(h, pose, on_device, peer_loop ? kPeerPace : kLsqPace, "vgicp: the optimiser did not finish within its pass budget", device_pass, host_pass, &r, shard,
                a.roi.escapes /* nullptr unless the target was prepared for one scan */))
        return 1;
    // some pass looked up a voxel outside the region the target was prepared for: its sums lack that correspondence.  The caller
    // prepares the whole target and repeats the call (2).
    if (h->roi_on && r.roi_escapes > 0) { h->roi_repeats += 1; return 2; }
    if (r.on_device) h->stats.attempts = r.passes;      // (the passes the device loop evaluated)
    uint32_t esc = 0;
    if (a.escapes) {
        H_TRY(hipMemcpyAsync(&esc, a.escapes, sizeof esc, hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        // the scan reaches (the reach of a covariance of) a face the index was cut at: 3 -- the caller cuts the target around THIS scan
        // and repeats (vgicp_align_recut).  A rank of a sharded call cannot, and must not leave either (its peers would wait in their
        // next collective): the count travels with the fitness sums below and every rank fails the call.
        if (esc && !shard) { h->err = "the target is too spread out for the dense voxel tables (a stray point far from the map?) and was cut to its bulk, but the scan reaches "
                                      "the part that was left out"; return 3; }
    }
    lsq_report(h, r, n_src, pose, converged);
    if (!shard) { arm_fitness(h, pose, n_src, stride_floats); return 0; }
    // sharded: every rank takes part in the sum, so the score is evaluated here, with the call (VgicpRegister.cpp:42-45)
    h->seq += 1.0;
    FitTile ft;
    memset(&ft, 0, sizeof ft);
    if (h->use_tile) {
        ft.use = 1;
        for (int d = 0; d < 3; ++d) { ft.lo[d] = h->tile_lo[d]; ft.hi[d] = h->tile_hi[d]; ft.ext_lo[d] = -1e300; ft.ext_hi[d] = 1e300; }
        if (h->have_halo) shard_extent(h, ft.ext_lo, ft.ext_hi);
    }
    H_TRY(fitness_launch(h->grid, d_src, n_src, stride_floats, pose, DBL_MAX, h->vg_partials.as<double>(), h->out32.dev, h->stream, h->seq,
                         h->use_tile ? &ft : nullptr));
    if (wait_result(h, &h->out32.host[31], h->seq)) return 1;
    h->out32.host[3] = (double)esc;      // (this rank's scan points that reached a cut face of its index)
    if (shard && ranks_allreduce(h, h->out32.host, 4)) return 1;
    if (h->out32.host[3] > 0) { h->err = "a rank's target is too spread out for the dense voxel tables (a stray point far from the map?) and was cut to its bulk, but the scan reaches "
                                         "the part that was left out"; return 3; }
    h->fitness = h->out32.host[1] > 0 ? h->out32.host[0] / h->out32.host[1] : DBL_MAX;
    // sharded: a source point farther from every map point than its rank's halo has its nearest neighbour on another rank; the
    // score is then not the map's and is reported as unavailable (the pose is unaffected)
    if (h->use_tile && h->out32.host[2] > 0) h->fitness = -1.0;
    return 0;
}

}  // namespace

namespace pcr {
namespace host {

// run_vgicp, and when the scan reached a cut face of an index that could not hold the whole target (a stray point kilometres away,
// a second cluster far off): the target cut around the scan itself -- its box at the initial pose plus the reach of a covariance plus
// room to move, doubled for as long as the scan still reaches a cut face -- and the alignment again from the same guess.  The
// reference's hash map and kd-tree serve any extent (fast_vgicp_voxel.hpp:129-156); with this a dense table does too, wherever the
// scan is.  d_dst: the target's points (the caller's buffer of a scan2map call, the staged copy of pcr_set_target, a sub-map).
int vgicp_align_recut(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) {
    double pose_in[16];
    memcpy(pose_in, pose, sizeof pose_in);
    int rc = run_vgicp(h, d_src, n_src, stride_floats, pose, converged);
    if (rc != 3) return rc;
    if (sharded(h)) return 1;      // (h->err says what happened)
    const double reach = std::max(4.0, 8.0 * h->prm.vgicp_resolution);
    h->clamp_margin = reach + kClampMargin;
    for (int attempt = 0; attempt < kClampRetries && rc == 3; ++attempt) {
        memcpy(pose, pose_in, sizeof pose_in);
        if (set_clamp_from_scan(h, d_src, n_src, stride_floats, pose_in)) return 1;
        if (vgicp_prepare_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride, nullptr, true)) return 1;
        rc = run_vgicp(h, d_src, n_src, stride_floats, pose, converged);
        h->clamp_margin *= 2.0;
    }
    if (rc == 3) return fail(h, "the pose left every region the target could be indexed over (a target too sparse for dense voxel tables and an optimiser that wanders)");
    return rc;
}

// ---- vgicp's row of the method table (handle.h: MethodOps) ----
int vgicp_scan2map(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged) {
    // the reference keeps its target structures while the cloud POINTER is unchanged and goes stale
    // when the cloud is edited in place; this entry point always rebuilds them
    // (source side first: its ~15 launches run on the side stream while the host is still queueing the target's.  Measured the other
    //  way round -- target builds queued first, source side enqueued while the host waits for them -- 1.17 instead of 0.93 ms: the
    //  two covariance kernels then run side by side for their whole length and slow each other down)
    // The target exists for this scan only, so only the part of it the scan can reach is prepared (RoiView): the covariances of a
    // 1 M-point map were 0.4 of a 0.85 ms call, of which the scan looks up a tenth.  Should the optimiser carry the scan out of that
    // region, the whole target is prepared and the call repeated from the same guess.
    const bool use_roi = !sharded(h) && n_src > 0 && h->prm.host_optimiser == 0 && h->prm.vgicp_max_iters > 0 && h->prm.full_target == 0;
    double pose_in[16];
    memcpy(pose_in, pose, sizeof pose_in);
    const RoiScan rs{d_src, n_src, stride_floats, pose_in};
    // Order of the two sides.  The scan's own covariances used to be the longest thing in a call (344 us) and were queued first; since
    // they are searched in two classes (cov_search.hip: ~190 us with the scan's index levels) the target is the long pole, and the
    // dozen launches of the scan's side cost the host ~100 us during which the main stream sat empty.  Now the target's builds are
    // queued first and the scan's side while the host waits for their headers (settle_cov_levels: before_wait).
    // (Measured and not kept: the scan's side queued by a host thread of its own at the same time as the target's -- 0.481 / 0.495 against
    //  0.496 / 0.494 ms: with both sides on the device from the start the call is bound by the device's work, not by the host's launches.)
    bool src_queued = false;
    const std::function<int()> queue_src = [&]() -> int { src_queued = true; return vgicp_source_enqueue(h, d_src, n_src, stride_floats, true); };
    int prc = vgicp_source_mark(h);
    if (!prc) prc = vgicp_prepare_target(h, d_dst, n_dst, stride_floats, use_roi ? &rs : nullptr, false, &queue_src);
    if (!prc && !src_queued) prc = queue_src();
    if (prc) (void)side_drain(h);
    if (agree_prepared(h, prc)) {
        (void)side_drain(h);
        return 1;
    }
    if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_index, h->stream));
    int rrc = vgicp_align_recut(h, d_src, n_src, stride_floats, pose, converged);
    if (rrc == 2) {
        memcpy(pose, pose_in, sizeof pose_in);
        if (vgicp_prepare_target(h, d_dst, n_dst, stride_floats, nullptr)) return 1;
        rrc = vgicp_align_recut(h, d_src, n_src, stride_floats, pose, converged);
    }
    if (rrc) return 1;
    return end_timed_call(h);
}
int vgicp_kept_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) { return agree_prepared(h, vgicp_prepare_target(h, d_dst, n_dst, stride_floats)); }
int align_beside_scan_side(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged, AlignFn* run) {
    // the scan's own side (two index levels, the 20-neighbour search, the covariances) queued on the side stream with its headers mirrored to the host, as
    // pcr_scan2map queues it -- unless pcr_scan2map_submap has queued it already, ahead of the target's preparation.  Settled the checked way (a header
    // read back after every level: two host round trips with an idle device in between, ~55 us of a 0.3 ms call against a kept sub-map) only if that fails.
    if (!sharded(h) && n_src > 0 && !(h->side_pending && h->side_src == d_src && h->side_n == n_src && h->side_stride == stride_floats) &&
        vgicp_source_enqueue(h, d_src, n_src, stride_floats)) return 1;
    const int rc = run(h, d_src, n_src, stride_floats, pose, converged) ? 1 : 0;
    (void)side_drain(h);      // (an alignment that failed before it collected the scan's side: nothing stays in flight behind the caller's back)
    return rc;
}
int vgicp_align(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) { return align_beside_scan_side(h, d_src, n_src, stride_floats, pose, converged, vgicp_align_recut); }
// the resolution is the voxel; the regularisation shaped every covariance the handle holds, the voxel mode the voxel map
bool vgicp_target_from_changed(const pcr_params& old_p, const pcr_params& new_p) { return new_p.vgicp_resolution != old_p.vgicp_resolution || new_p.vgicp_regularization != old_p.vgicp_regularization || new_p.vgicp_voxel_mode != old_p.vgicp_voxel_mode; }

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_vgicp_covariances(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double* cov_out) {
    if (!h) return 1;
    h->err.clear();
    if (!vgicp_family(h)) return fail(h, "pcr_vgicp_covariances needs a vgicp or gicp handle");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    const float* d_pts = (const float*)pts;
    if (!on_device && stage_host(h, &h->src_stage, pts, n, stride_bytes, &d_pts)) return 1;
    H_TRY(side_drain(h));
    if (settle_scan_levels(h, d_pts, n, stride_bytes / 4)) return 1;
    H_TRY(h->vg.src_cov6.reserve((n + 1) * 6 * sizeof(double)));
    H_TRY(hipMemsetAsync(h->vg.src_cov6.p, 0, (n + 1) * 6 * sizeof(double), h->stream));
    H_TRY(vgicp_launch_cov(h->src_grid, cov_levels(n) > 1 ? &h->vg.src_l1 : nullptr, cov_levels(n) > 2 ? &h->vg.src_l2 : nullptr, d_pts, stride_bytes / 4, n,
                           h->vg.src_cov6.as<double>(), h->stream, h->prm.vgicp_regularization, nullptr, nullptr, &h->vg.src_scratch));
    H_TRY(hipMemcpyAsync(cov_out, h->vg.src_cov6.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int pcr_vgicp_neighbours(pcr_handle* h, size_t n, uint32_t* nbr_out, uint32_t* queued_out) {
    if (!h) return 1;
    h->err.clear();
    if (!vgicp_family(h)) return fail(h, "pcr_vgicp_neighbours needs a vgicp or gicp handle");
    if (set_device(h)) return 1;
    const CovScratch& sc = h->vg.src_scratch;
    if (!sc.nbr.p || !h->src_grid.valid || h->src_grid.n_points > n || !scan_sized(n)) return fail(h, "no neighbour lists of a cloud of that size: call pcr_vgicp_covariances on a scan-sized cloud first");
    const size_t n_cap = std::min(sc.queue.cap / sizeof(uint32_t), sc.nbr.cap / (20 * sizeof(uint32_t))), ns = h->src_grid.n_points;
    std::vector<uint32_t> lists(n_cap * 20);
    std::vector<float> sorted(ns * 4);
    uint32_t queued = 0;
    H_TRY(hipStreamSynchronize(h->stream));
    H_TRY(hipMemcpy(lists.data(), sc.nbr.p, lists.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    H_TRY(hipMemcpy(sorted.data(), h->src_grid.sorted.p, sorted.size() * sizeof(float), hipMemcpyDeviceToHost));
    H_TRY(hipMemcpy(&queued, sc.count.p, sizeof queued, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n * 20; ++i) nbr_out[i] = 0xffffffffu;
    for (size_t j = 0; j < ns; ++j) {
        uint32_t orig;
        memcpy(&orig, &sorted[j * 4 + 3], 4);
        if (orig >= n) return fail(h, "the scan index does not belong to a cloud of that size");
        for (int k = 0; k < 20; ++k) nbr_out[(size_t)orig * 20 + k] = lists[(size_t)k * n_cap + j];
    }
    if (queued_out) *queued_out = queued;
    return 0;
}

int pcr_vgicp_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double pose[16],
                        double H[36], double b[6], double* error, int64_t* n_corr) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kVgicp) return fail(h, "pcr_vgicp_linearize needs a vgicp handle");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->target_ready) return fail(h, "no target: call pcr_set_target first");
    if (ensure_full_target(h)) return 1;
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    // run the driver's set-up with zero iterations, then one linearisation at the given pose
    const int saved = h->prm.vgicp_max_iters;
    h->prm.vgicp_max_iters = 0;
    double tmp[16];
    memcpy(tmp, pose, sizeof tmp);
    int conv = 0;
    const int rc = run_vgicp(h, d_src, n_src, stride_bytes / 4, tmp, &conv);
    h->prm.vgicp_max_iters = saved;
    if (rc) return 1;
    Pose16 T;
    memcpy(T.m, pose, sizeof T.m);
    H_TRY(vgicp_launch_linearize(vgicp_args(h, d_src, n_src, stride_bytes / 4), T, h->out32.dev, h->stream));
    // the pairs: DIRECT1 one slot per point, DIRECT7 / DIRECT27 the K rows of slots (VgicpArgs::corr_slot; the presence bits behind them are not counted)
    const size_t n_entries = vgicp_table_entries(h->prm.vgicp_search);
    std::vector<uint32_t> slots(n_src * n_entries);
    if (n_src) H_TRY(hipMemcpyAsync(slots.data(), h->vg.corr_slot.p, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    if (sharded(h) && ranks_allreduce(h, h->out32.host, 29)) return 1;
    unpack_lsq_sums(h->out32.host, H, b, error);
    if (n_corr) { int64_t c = 0; for (uint32_t v : slots) c += v != 0; *n_corr = c; }
    h->vg.lin_valid = true; h->vg.lin_n = n_src; h->vg.lin_search = h->prm.vgicp_search;
    return 0;
}

int pcr_vgicp_correspondences(pcr_handle* h, pcr_vgicp_corr* out, size_t capacity, size_t* count) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kVgicp) return fail(h, "pcr_vgicp_correspondences needs a vgicp handle");
    if (set_device(h)) return 1;
    if (!h->vg.lin_valid || !h->target_ready || h->roi_on) return fail(h, "pcr_vgicp_correspondences: no linearisation to report; call pcr_vgicp_linearize first");
    const size_t n_src = h->vg.lin_n, n_entries = vgicp_table_entries(h->vg.lin_search);
    H_TRY(hipStreamSynchronize(h->stream));
    GridHeader hd;
    H_TRY(hipMemcpy(&hd, h->grid.header.p, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.overflow || hd.stale) return fail(h, "internal: the index of a target that pcr_set_target settled is incomplete");
    size_t pairs = 0;
    if (!hd.empty && n_src) {
        std::vector<uint32_t> slots(n_src * n_entries), start((size_t)hd.n_cells + 1);
        H_TRY(hipMemcpy(slots.data(), h->vg.corr_slot.p, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        H_TRY(hipMemcpy(start.data(), h->grid.cell_start.p, start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const uint32_t d0 = (uint32_t)hd.dims[0], d1 = (uint32_t)hd.dims[1];
        for (size_t i = 0; i < n_src; ++i)
            for (size_t k = 0; k < n_entries; ++k) {
                const uint32_t slot = slots[k * n_src + i];      // ([K][n_src]; DIRECT1: [n_src])
                if (!slot) continue;
                if (out && pairs < capacity) {
                    // a voxel is stored at the position of its cell's first point: the cell is the LAST one that starts there (the empty cells in front of it start there too)
                    const size_t t = (size_t)(std::upper_bound(start.begin(), start.end(), slot - 1u) - start.begin()) - 1;
                    if (t >= (size_t)hd.n_cells || start[t] != slot - 1u) return fail(h, "internal: a correspondence that is no voxel of the target");
                    const uint32_t row = (uint32_t)(t / d0), cz = row / d1;
                    pcr_vgicp_corr& o = out[pairs];
                    o.row = (int32_t)i;
                    o.ijk[0] = (int32_t)((uint32_t)t - row * d0) + (int32_t)hd.org[0]; o.ijk[1] = (int32_t)(row - cz * d1) + (int32_t)hd.org[1]; o.ijk[2] = (int32_t)cz + (int32_t)hd.org[2];
                }
                ++pairs;
            }
    }
    if (count) *count = pairs;
    if (out && capacity < pairs) return fail(h, "pcr_vgicp_correspondences: room for " + std::to_string(capacity) + " pairs, the linearisation has " + std::to_string(pairs));
    return 0;
}

/* ---- read-only introspection for the test suite: not called by pcr_scan2map / pcr_align ---- */
int pcr_vgicp_voxels(pcr_handle* h, pcr_vgicp_voxel* out, size_t capacity, size_t* count) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kVgicp) return fail(h, "pcr_vgicp_voxels needs a vgicp handle");
    if (set_device(h)) return 1;
    if (!h->target_ready) return fail(h, "no target: call pcr_set_target first");
    if (h->roi_on) return fail(h, "pcr_vgicp_voxels: pcr_scan2map prepared this target for that one scan's region only; call pcr_set_target first, for a target that is kept");
    H_TRY(hipStreamSynchronize(h->stream));
    GridHeader hd;
    H_TRY(hipMemcpy(&hd, h->grid.header.p, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.overflow || hd.stale) return fail(h, "internal: the index of a target that pcr_set_target settled is incomplete");
    // a voxel is a cell of the index, stored at the position of the cell's first point (vgicp.hip: vgicp_voxel_kernel)
    size_t kept = 0;
    if (!hd.empty) {
        std::vector<uint32_t> start((size_t)hd.n_cells + 1);
        H_TRY(hipMemcpy(start.data(), h->grid.cell_start.p, start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const size_t n = start[hd.n_cells];
        std::vector<VgicpVoxel> vox(out ? n : 0);
        if (out && n) H_TRY(hipMemcpy(vox.data(), h->vg.vox.p, n * sizeof(VgicpVoxel), hipMemcpyDeviceToHost));
        const uint32_t d0 = (uint32_t)hd.dims[0], d1 = (uint32_t)hd.dims[1];
        for (size_t t = 0; t < (size_t)hd.n_cells; ++t) {
            if (start[t + 1] <= start[t]) continue;
            if (out && kept < capacity) {
                const uint32_t row = (uint32_t)(t / d0), cz = row / d1;
                const VgicpVoxel& v = vox[start[t]];
                pcr_vgicp_voxel& o = out[kept];
                // the lattice coordinate floor(p / res - 0.5): the cell's position in the box + the box's origin
                o.ijk[0] = (int32_t)((uint32_t)t - row * d0) + (int32_t)hd.org[0]; o.ijk[1] = (int32_t)(row - cz * d1) + (int32_t)hd.org[1]; o.ijk[2] = (int32_t)cz + (int32_t)hd.org[2];
                o.n = (int32_t)v.n;
                memcpy(o.mean, v.mean, sizeof o.mean);
                memcpy(o.cov, v.cov, sizeof o.cov);
            }
            ++kept;
        }
    }
    if (count) *count = kept;
    if (out && capacity < kept) return fail(h, "pcr_vgicp_voxels: room for " + std::to_string(capacity) + " voxels, the target has " + std::to_string(kept));
    return 0;
}

struct pcr_vgicp_opt { VgCtl c; };

pcr_vgicp_opt* pcr_vgicp_opt_create(const double pose_guess[16], int max_iters, int lm_inner, double lm_init_scale, double rot_eps, double trans_eps) {
    if (!pose_guess) return nullptr;
    pcr_vgicp_opt* o = new pcr_vgicp_opt;
    memset(&o->c, 0, sizeof o->c);
    Pose16 g;
    for (int i = 0; i < 16; ++i) g.m[i] = (double)(float)pose_guess[i];      // guess handed over as Matrix4f (VgicpRegister.cpp:36), as run_vgicp does
    vg_opt::ctl_init(&o->c, g, max_iters, lm_inner, lm_init_scale, rot_eps, trans_eps);
    return o;
}
void pcr_vgicp_opt_destroy(pcr_vgicp_opt* o) { delete o; }
int pcr_vgicp_opt_request(const pcr_vgicp_opt* o, int* kind, double pose_eval[16], double pose_lin[16]) {
    if (!o || !kind) return 1;
    *kind = o->c.done ? 2 : o->c.kind;
    if (pose_eval) for (int i = 0; i < 16; ++i) pose_eval[i] = o->c.xi.m[i];
    if (pose_lin) for (int i = 0; i < 16; ++i) pose_lin[i] = o->c.x0.m[i];
    return 0;
}
int pcr_vgicp_opt_feed(pcr_vgicp_opt* o, const double sums[29]) {
    if (!o || !sums || o->c.done) return 1;
    vg_opt::ctl_step(&o->c, sums);
    return 0;
}
int pcr_vgicp_opt_result(const pcr_vgicp_opt* o, double pose16[16], int* converged, int* outer_iterations, int* done) {
    if (!o) return 1;
    if (pose16) for (int i = 0; i < 16; ++i) pose16[i] = o->c.x0.m[i];
    if (converged) *converged = o->c.conv;
    if (outer_iterations) *outer_iterations = o->c.outer;
    if (done) *done = o->c.done;
    return 0;
}

}  // extern "C"
