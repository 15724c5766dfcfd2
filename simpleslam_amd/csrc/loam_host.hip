// loam_host.hip -- LOAM host driver: the target index and its sizing (a box that cannot be tabulated is cut: ClampBox), the
// launch sequence of an alignment (LoamRegister.cpp:110-220), pcr_loam_linearize and the trace / timeline read-outs.

#include <algorithm>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace {

double grid_cell_for(double max_sq) {
    // smallest power of two >= the gate radius, so that x / cell is exact in f64
    double r = sqrt(max_sq > 0 ? max_sq : 1.0), c = 1.0;
    while (c < r) c *= 2.0;
    while (c * 0.5 >= r) c *= 0.5;
    return c;
}

int ensure_loam_buffers(pcr_handle* h) {
    H_TRY(h->loam.state.reserve(2 * sizeof(LoamState)));
    H_TRY(h->loam.partials.reserve((size_t)2 * kMaxPartials * kAccum * sizeof(double)));
    H_TRY(h->loam.reduced.reserve(kAccum * sizeof(double)));
    const int iters = std::max(1, h->prm.loam_iters);
    if (h->prm.record_trace) H_TRY(h->loam.trace.reserve((size_t)iters * sizeof(LoamTrace)));
    H_TRY(h->loam.result.ensure());
    if (h->comm.host_ar) H_TRY(h->loam.red.ensure(kAccum));
    return 0;
}

void fill_loam_args(pcr_handle* h, LoamArgs* a, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16]) {
    memset(a, 0, sizeof(*a));
    a->src = d_src; a->n_src = (uint32_t)n_src; a->src_stride = (uint32_t)stride_floats;
    a->grid = h->grid.view();
    a->c.knn_max_sq = h->prm.loam_knn_max_sq; a->c.plane_thresh = h->prm.loam_plane_thresh;
    a->c.point_thresh = h->prm.loam_point_thresh; a->c.pos_conv = h->prm.loam_pos_conv; a->c.rot_conv = h->prm.loam_rot_conv;
    a->c.iters = h->prm.loam_iters; a->c.early_exit = h->prm.loam_early_exit;
    memcpy(a->init_pose, pose, 16 * sizeof(double));
    a->state = h->loam.state.as<LoamState>();
    a->partials = h->loam.partials.as<double>();
    a->reduced = nullptr;
    a->n_partials = loam_grid_blocks((uint32_t)n_src);
    h->loam.last_blocks = a->n_partials;
    a->trace = h->prm.record_trace ? h->loam.trace.as<LoamTrace>() : nullptr;
    a->result = h->loam.result.dev;
    a->coresident = h->prm.loam_coresident == 1;
    if (h->prm.loam_disable_cache == 0 && h->loam.nn_cache.reserve(loam_cache_bytes(n_src)) == hipSuccess) a->nn_cache = h->loam.nn_cache.as<float4>();
    if (h->prm.record_timeline == 1 && h->loam.timeline.reserve((size_t)(std::max(1, h->prm.loam_iters) + 1) * kMaxPartials * kTimelineSlots * sizeof(unsigned long long)) == hipSuccess)
        a->timeline = h->loam.timeline.as<unsigned long long>();
    a->use_tile = h->use_tile;
    for (int d = 0; d < 3; ++d) { a->tile_lo[d] = h->tile_lo[d]; a->tile_hi[d] = h->tile_hi[d]; }
}

}  // namespace

namespace pcr {
namespace host {

int build_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) {
    double cell = 1.0;
    if (h->method == kLoam) cell = grid_cell_for(h->prm.loam_knn_max_sq);
    // (the bounding box of the previous target is tried first: GridIndex::hint_ok -- unless pcr_params.index_no_hints)
    h->grid.no_hints = h->prm.index_no_hints != 0;
    hipError_t e = h->grid.build(d_dst, n_dst, stride_floats, cell, h->stream, &h->err, 0.0, 0, h->clamp.use ? &h->clamp : nullptr, h->method == kLoam);
    if (e != hipSuccess) return 1;
    h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats; h->have_target = true;
    return 0;
}
// The box taken over from the previous target does not hold this one (header.stale): the kept target again, with a fresh box, padded from now on.
int rebuild_stale_target(pcr_handle* h) {
    h->grid.hint_margin = 8; h->grid.cells_hint = 0;      // (a cloud that left the old box: its cell count is anybody's guess too)
    return build_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride);
}

// After a synchronisation: did the device-side build overflow the cell table?  Then grow and rebuild.
// Returns 0 ok (no overflow), 2 rebuilt (caller must rerun), 1 error.
// Dense tables stop at 4e9 cells.  A cloud that needs more -- a stray point kilometres away from the map -- is refused,
// except where the caller's scan tells which part of it can matter: LOAM scan2map then indexes only the target points
// within clamp_margin of the scan as the initial pose places it (a query only ever looks one gate radius around itself;
// the margin is the room the pose has to move during the iterations).  The kernels count the queries that come within a
// cell of a cut face (LoamState.fail == 3): such a call is redone on a region twice as wide, so the result is the full
// index's whenever the call succeeds.  (kClampMargin, kClampRetries: handle.h -- vgicp_align_recut widens by them too.)

int set_clamp_from_scan(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16]) {
    if (!n_src) return fail(h, "target bounding box too large for the dense index and the scan is empty");
    // bounding box of the scan: one index build over it (rare path), read back from its header
    if (h->src_grid.build(d_src, n_src, stride_floats, 1.0, h->stream, &h->err) != hipSuccess) return 1;
    GridHeader sh;
    H_TRY(hipMemcpyAsync(&sh, h->src_grid.header.p, sizeof sh, hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    if (sh.empty) return fail(h, "target bounding box too large for the dense index and the scan has no finite point");
    double lo[3], hi[3], mlo[3] = {1e300, 1e300, 1e300}, mhi[3] = {-1e300, -1e300, -1e300};
    for (int d = 0; d < 3; ++d) { lo[d] = sh.origin[d]; hi[d] = sh.origin[d] + sh.dims[d] * sh.cell; }      // a superset of the scan's box
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2]};
        for (int r = 0; r < 3; ++r) {
            const double v = pose[r] * p[0] + pose[4 + r] * p[1] + pose[8 + r] * p[2] + pose[12 + r];
            mlo[r] = std::min(mlo[r], v); mhi[r] = std::max(mhi[r], v);
        }
    }
    for (int d = 0; d < 3; ++d) {
        if (!(mlo[d] == mlo[d] && mhi[d] == mhi[d])) return fail(h, "target bounding box too large for the dense index and the initial pose is not finite");
        h->clamp.lo[d] = mlo[d] - h->clamp_margin; h->clamp.hi[d] = mhi[d] + h->clamp_margin;
    }
    h->clamp.use = 1;
    return 0;
}

// pcr_set_target on a cloud whose bounding box cannot be tabulated (a stray point kilometres away) and no scan to cut the box around:
// the box of the BULK of the cloud instead.  A strided sample of <= 4096 points comes to the host; per axis the 2nd and 98th
// percentile of the finite samples, widened by half their span + 20 m, is a region that holds every point of an ordinary map and
// leaves a stray one out.  What lies outside is not indexed -- and, as with the scan-centred cut, not silently: a face with target
// points beyond it is marked (header.cut_mask), a query whose 3x3x3 block touches such a face is counted, and the registration is
// then redone on a region cut around the scan (run_loam), so a scan that really visits the far part of the cloud is still served.
int set_clamp_from_target_sample(pcr_handle* h, bool room) {
    const size_t n = h->tgt_n, stride_b = h->tgt_stride * 4;
    if (!n || !h->tgt_ptr) return fail(h, "target bounding box too large for the dense index");
    const size_t step = std::max<size_t>(1, n / 4096), m = (n + step - 1) / step;
    std::vector<float> xyz(m * 3);
    H_TRY(hipMemcpy2DAsync(xyz.data(), 12, h->tgt_ptr, stride_b * step, 12, m, hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    for (int d = 0; d < 3; ++d) {
        std::vector<double> v;
        v.reserve(m);
        for (size_t i = 0; i < m; ++i) { const float a = xyz[i * 3], b = xyz[i * 3 + 1], c = xyz[i * 3 + 2]; if (std::isfinite(a) && std::isfinite(b) && std::isfinite(c)) v.push_back((double)xyz[i * 3 + d]); }
        if (v.empty()) return fail(h, "target bounding box too large for the dense index and no finite point in its sample");
        std::sort(v.begin(), v.end());
        const double q_lo = v[(size_t)(0.02 * (double)(v.size() - 1))], q_hi = v[(size_t)(0.98 * (double)(v.size() - 1) + 0.5)];
        const double pad = 0.5 * (q_hi - q_lo) + 20.0;
        h->clamp.lo[d] = q_lo - pad; h->clamp.hi[d] = q_hi + pad;
    }
    // room: the index over the bulk box has itself reported more cells than a dense table can have, at the cell the caller builds with (two
    // sessions 30 km apart: the percentiles span both; such a target was refused).  Then the room around ONE point of the cloud -- the finite
    // sample whose x is the median -- 500 m x 500 m x 200 m: an index that can be built, cut faces that are marked as above, and a registration
    // elsewhere in the cloud redone on a region cut around its scan.  (pcr_knn / pcr_radius_search answer such a target from the sparse index.)
    if (room) {
        std::vector<size_t> fin;
        for (size_t i = 0; i < m; ++i) if (std::isfinite(xyz[i * 3]) && std::isfinite(xyz[i * 3 + 1]) && std::isfinite(xyz[i * 3 + 2])) fin.push_back(i);
        std::nth_element(fin.begin(), fin.begin() + fin.size() / 2, fin.end(), [&](size_t a, size_t b) { return xyz[a * 3] != xyz[b * 3] ? xyz[a * 3] < xyz[b * 3] : a < b; });
        const size_t c = fin[fin.size() / 2];
        const double half[3] = {250.0, 250.0, 100.0};
        for (int d = 0; d < 3; ++d) { h->clamp.lo[d] = (double)xyz[c * 3 + d] - half[d]; h->clamp.hi[d] = (double)xyz[c * 3 + d] + half[d]; }
    }
    h->clamp.use = 1;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

int check_grid_overflow(pcr_handle* h, int overflow, uint64_t need_cells, const float* d_src = nullptr, size_t n_src = 0, size_t stride_floats = 0,
                        const double* pose = nullptr) {
    if (!overflow) return 0;
    if (need_cells > 4000000000ull && h->method == kLoam && d_src && pose && !h->clamp.use) {
        if (set_clamp_from_scan(h, d_src, n_src, stride_floats, pose)) return 1;
        if (build_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride)) return 1;
        return 2;
    }
    if (need_cells > 4000000000ull && h->method == kLoam && h->clamp_from_bulk && h->clamp_bulk_stage < 2) {      // pcr_set_target: no scan to go by
        // the bulk of the cloud first; when the index over THAT box reports more than 4e9 cells too, the room around one point of it
        if (set_clamp_from_target_sample(h, h->clamp_bulk_stage == 1)) return 1;
        h->clamp_bulk_stage += 1;
        if (build_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride)) return 1;
        return 2;
    }
    if (h->grid.grow_cells(need_cells, &h->err) != hipSuccess) return 1;
    if (build_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride)) return 1;
    return 2;
}

}  // namespace

namespace pcr {
namespace host {

// Bring the enqueued index build to a usable state before anything else is launched: read the header back and grow the
// cell table (or cut the box around the scan) until it fits.  No collective in here -- a sharded call settles its tile
// on every rank independently and only then enters the exchange loop (a rank that retried on its own after the loop, as the
// unsharded path does, would leave the other ranks' all-reduces without a peer).
int settle_loam_index(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, const double* pose) {
    for (int attempt = 0; attempt < 6; ++attempt) {
        GridHeader hdr;
        H_TRY(hipMemcpyAsync(&hdr, h->grid.header.p, sizeof(hdr), hipMemcpyDeviceToHost, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        if (hdr.stale) {
            if (rebuild_stale_target(h)) return 1;
            continue;
        }
        const int ov = check_grid_overflow(h, hdr.overflow, hdr.n_cells, h->clamp_allowed ? d_src : nullptr, n_src, stride_floats, pose);
        if (ov == 0) { if (!hdr.empty) { h->grid.confirm(); h->grid.note_cells(hdr.n_cells); } return 0; }      // (the header of an EMPTY target is no hint: the kernels of a build that reused it would leave at once)
        if (ov == 1) return 1;
    }
    return fail(h, "target index could not be sized");
}

int run_loam(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged,
             bool index_timed) {
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    if (peer_check(h)) return 1;
    if (ensure_loam_buffers(h)) return 1;
    const int iters = std::max(0, h->prm.loam_iters);
    const bool shard = sharded(h);
    // (pcr_params.loam_clamp_margin_mm: first margin in millimetres, a test hook that makes the widening path reachable with ordinary clouds)
    // (may be negative: the scan's box is padded by two index cells already, so only a region cut INTO the scan makes queries reach its edge)
    h->clamp_margin = h->prm.loam_clamp_margin_mm != 0 ? 1e-3 * h->prm.loam_clamp_margin_mm : kClampMargin;
    const double margin_cap = kClampMargin * (1 << kClampRetries);
    for (int attempt = 0; attempt < 24; ++attempt) {
        bool rank_fail = false;
        std::string rank_err;
        if (shard) {
            // The exchange loop below must run the same number of collectives on every rank whatever happens to this rank's
            // index: settle it first, and if that fails take part with empty sums and a flag that stops all ranks together.
            if (!h->grid.valid || settle_loam_index(h, d_src, n_src, stride_floats, pose)) {
                rank_fail = true; rank_err = h->err.empty() ? "target index not built" : h->err;
                if (!h->loam.dummy_grid.p) {
                    GridHeader dh;
                    memset(&dh, 0, sizeof dh);
                    dh.overflow = 1; dh.empty = 1; dh.cell = dh.inv_cell = 1.0; dh.n_cells = 1;
                    // (the header is followed by a few zero words that stand in for the cell table and the point array)
                    if (h->loam.dummy_grid.reserve(sizeof dh + 1024) != hipSuccess || hipMemset(h->loam.dummy_grid.p, 0, sizeof dh + 1024) != hipSuccess ||
                        hipMemcpy(h->loam.dummy_grid.p, &dh, sizeof dh, hipMemcpyHostToDevice) != hipSuccess)
                        return fail(h, rank_err + " (and no memory for the stand-in header: the other ranks of this call will hang)");
                }
            }
        }
        LoamArgs a;
        fill_loam_args(h, &a, d_src, n_src, stride_floats, pose);
        if (rank_fail) {
            a.grid.hdr = h->loam.dummy_grid.as<GridHeader>();
            a.grid.pts = reinterpret_cast<const float4*>(h->loam.dummy_grid.as<char>() + 512);
            a.grid.cell_start = reinterpret_cast<const uint32_t*>(h->loam.dummy_grid.as<char>() + 512);
            a.rank_fail = 1; a.nn_cache = nullptr;
        }
        if (shard) a.reduced = h->comm.host_ar ? h->loam.red.dev : h->loam.reduced.as<double>();
        h->loam.result.host->pad = 0;
        if (h->profile >= 1 && !index_timed) { H_TRY(hipEventRecord(h->ev_start, h->stream)); H_TRY(hipEventRecord(h->ev_index, h->stream)); }
        const bool per_kernel = h->profile >= 2;
        if (per_kernel) {
            while ((int)h->ev_kernel.size() < 2 * iters) { hipEvent_t e; H_TRY(hipEventCreate(&e)); h->ev_kernel.push_back(e); }
        }
        // Early exit (the reference's default: LoamRegister.cpp:198-220 leaves the loop once a step is small): the device ends the loop in a launch's
        // prologue and the launches behind it leave at once -- but each still costs ~5 us of the stream, and the caller's loop converges after two
        // iterations of eight (extra.sequence).  So with early exit on, the host stays TWO launches ahead of the prologue's progress word (host-mapped)
        // instead of queueing all of them: a loop that ends after launch 2 costs four launches, not eight.  Without early exit (BASELINE's ten fixed
        // iterations), sharded, or timed per kernel: everything is queued at once, as before.
        const bool paced = a.c.early_exit != 0 && !shard && !per_kernel && iters > 3;
        volatile int32_t* const progress = &h->loam.result.host->progress;
        *progress = -1;
        int launched = 0;
        for (int k = 0; k < iters; ++k) {
            if (paced && k >= 3) {
                const int32_t want = (int32_t)(k - 2) << 1;
                int32_t v = *progress;
                for (int spin = 0; spin < 400000 && v < want; ++spin) { __builtin_ia32_pause(); v = *progress; }      // (bounded: a stalled device gets the launch anyway)
                if (v >= 0 && (v & 1)) break;
            }
            ++launched;
            if (per_kernel) H_TRY(loam_launch_iteration(a, k, h->stream, h->ev_kernel[2 * k], h->ev_kernel[2 * k + 1]));
            else H_TRY(loam_launch_iteration(a, k, h->stream));
            if (h->comm.host_ar) {
                // the caller's collective: sums to the host, through fn, back (one host round trip per linearisation)
                H_TRY(loam_launch_reduce(a, k, h->loam.red.dev, h->stream));
                H_TRY(hipStreamSynchronize(h->stream));
                if (ranks_allreduce(h, h->loam.red.host, kAccum)) return 1;
            } else if (h->comm.peer_on) {
                // fold + push to every peer + fold what arrived, one launch (the sums never leave the device)
                h->comm.peer_seq += 1.0;
                H_TRY(loam_launch_peer_exchange(a, k, h->comm.peer, h->comm.peer_seq, h->loam.reduced.as<double>(), h->stream));
            } else if (h->comm.rccl) {
                H_TRY(loam_launch_reduce(a, k, h->loam.reduced.as<double>(), h->stream));
                if (rccl_sum(h, h->loam.reduced.p, kAccum)) return 1;
            }
        }
        H_TRY(loam_launch_finalize(a, launched, h->stream));
        if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_end, h->stream));
        // The result arrives in host-mapped memory, its completion word written last with a system-scope release: a short
        // spin on that word returns a few microseconds before the stream's completion signal wakes a sleeping thread
        // (a frontend thread is waiting for this pose anyway).  Timing with events, or a slow call, falls back to the sync.
        if (h->profile == 0) {
            volatile int32_t* flag = &h->loam.result.host->pad;
            for (int spin = 0; spin < 200000 && *flag != 1; ++spin) __builtin_ia32_pause();
            std::atomic_thread_fence(std::memory_order_acquire);
            if (*flag != 1) H_TRY(hipStreamSynchronize(h->stream));
        } else {
            H_TRY(hipStreamSynchronize(h->stream));
        }
        const LoamResult r = *h->loam.result.host;
        if (r.pad != 1) return fail(h, "LOAM finalize kernel did not complete");
        if (peer_check(h)) return 1;      // (an exchange of this call timed out: the ranks that waited stopped their loops -- slot 30 -- and the session is over)
        if (r.fail == 2 || rank_fail)      // (every rank sees the flag in the sums of the first linearisation: all return here together)
            return fail(h, rank_fail ? "this rank could not index its map tile: " + rank_err : "sharded scan2map: another rank could not index its map tile");
        if (r.fail == 3) {
            // some query reached a face the index was cut at: the same call again, twice the room around the scan.  Sharded: all
            // ranks see the count in the same sums and come back here together, whether or not their own tile was cut.
            h->clamp_margin = std::max(2.0 * h->clamp_margin, h->clamp_margin + 1.0);
            if (h->clamp_margin > margin_cap) return fail(h, "the pose left the region of a target too sparse for the dense index (a stray point far from the map?)");
            if (h->clamp.use) {
                if (set_clamp_from_scan(h, d_src, n_src, stride_floats, pose)) { if (!shard) return 1; h->grid.valid = false; }
                else if (build_target(h, h->tgt_ptr, h->tgt_n, h->tgt_stride)) { if (!shard) return 1; }
            }
            index_timed = false;
            continue;
        }
        if (!shard) {
            if (r.grid_stale) {
                if (rebuild_stale_target(h)) return 1;
                index_timed = false;
                continue;
            }
            int ov = check_grid_overflow(h, r.grid_overflow, r.grid_cells, h->clamp_allowed ? d_src : nullptr, n_src, stride_floats, pose);
            if (ov == 1) return 1;
            if (ov == 2) { index_timed = false; continue; }
            if (!h->clamp.use && !r.grid_empty) { h->grid.confirm(); h->grid.note_cells(r.grid_cells); }      // (an empty target's header is no hint)
        }
        memcpy(pose, r.pose, 16 * sizeof(double));
        if (converged) *converged = r.converged;
        h->stats.iterations = r.iters_run; h->stats.attempts = attempt + 1;
        h->stats.n_src = (int64_t)n_src; h->stats.n_dst = (int64_t)h->tgt_n;
        h->stats.kernel_ms = 0; h->stats.kernel_launches = 0;
        if (h->profile >= 1 && read_call_times(h)) return 1;
        if (per_kernel) {
            // only launches that linearised count (the loop may have ended early)
            const int used = std::min(iters, r.converged || r.fail ? r.iters_run : iters);
            for (int k = 0; k < used; ++k) {
                float ms = 0;
                H_TRY(hipEventElapsedTime(&ms, h->ev_kernel[2 * k], h->ev_kernel[2 * k + 1]));
                h->stats.kernel_ms += ms; h->stats.kernel_launches++;
            }
        }
        if (h->prm.record_trace && iters > 0) {
            h->loam.trace_host.resize(iters);
            H_TRY(hipMemcpy(h->loam.trace_host.data(), h->loam.trace.p, (size_t)iters * sizeof(LoamTrace), hipMemcpyDeviceToHost));
            h->loam.trace_iters = r.iters_run;
        }
        return 0;
    }
    return fail(h, "target index could not be sized");
}

// ---- loam's row of the method table (handle.h: MethodOps) ----
int loam_scan2map(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged) {
    // the reference rebuilds its index on every call (LoamRegister.cpp:110); so do we
    h->clamp.use = 0;
    if (build_target(h, d_dst, n_dst, stride_floats)) {
        if (!sharded(h)) return 1;
        h->grid.valid = false;         // sharded: run_loam tells the other ranks and all of them fail together
        h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats;
    }
    if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_index, h->stream));
    h->clamp_allowed = true;           // this target exists for this scan only: a box that cannot be tabulated may be cut around it
    const int rc = run_loam(h, d_src, n_src, stride_floats, pose, converged, true);
    h->clamp_allowed = false;
    if (h->clamp.use) { h->clamp.use = 0; h->have_target = false; h->grid.valid = false; }      // not an index pcr_align may reuse
    return rc;
}
int loam_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) {
    h->clamp.use = 0;
    // settle the cell-table size now so that pcr_align never has to rebuild
    int rc = build_target(h, d_dst, n_dst, stride_floats);
    h->clamp_bulk_stage = 0;
    h->clamp_from_bulk = true;          // a box that cannot be tabulated is cut to the bulk of the cloud (set_clamp_from_target_sample)
    if (!rc) rc = settle_loam_index(h, nullptr, 0, 0, nullptr);
    h->clamp_from_bulk = false;
    if (rc) { h->have_target = false; h->grid.valid = false; }
    return agree_prepared(h, rc);
}
int loam_align(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) { return run_loam(h, d_src, n_src, stride_floats, pose, converged, false); }
// the gate sets the cell of the index
bool loam_target_from_changed(const pcr_params& old_p, const pcr_params& new_p) { return new_p.loam_knn_max_sq != old_p.loam_knn_max_sq; }

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_loam_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device,
                       const double pose[16], double JtJ[36], double JtE[6], int64_t* n_accepted, int8_t* status,
                       double* rows, int32_t* nn) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kLoam) return fail(h, "pcr_loam_linearize needs a loam handle");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->have_target || !h->grid.valid) return fail(h, "no target: call pcr_set_target first");
    if (ensure_loam_buffers(h)) return 1;
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    LoamArgs a;
    fill_loam_args(h, &a, d_src, n_src, stride_bytes / 4, pose);
    a.trace = nullptr;
    if (status) { H_TRY(h->loam.dbg_status.reserve(n_src + 16)); a.dbg_status = h->loam.dbg_status.as<int8_t>(); }
    if (rows) { H_TRY(h->loam.dbg_rows.reserve(n_src * 7 * sizeof(double) + 16)); a.dbg_rows = h->loam.dbg_rows.as<double>(); }
    if (nn) { H_TRY(h->loam.dbg_nn.reserve(n_src * 5 * sizeof(int32_t) + 16)); a.dbg_nn = h->loam.dbg_nn.as<int32_t>(); }
    H_TRY(loam_launch_iteration(a, 0, h->stream));
    H_TRY(loam_launch_reduce(a, 0, h->loam.reduced.as<double>(), h->stream));
    double sums[kAccum];
    H_TRY(hipMemcpyAsync(sums, h->loam.reduced.p, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
    if (status) H_TRY(hipMemcpyAsync(status, h->loam.dbg_status.p, n_src, hipMemcpyDeviceToHost, h->stream));
    if (rows) H_TRY(hipMemcpyAsync(rows, h->loam.dbg_rows.p, n_src * 7 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (nn) H_TRY(hipMemcpyAsync(nn, h->loam.dbg_nn.p, n_src * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    int q = 0;
    for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { JtJ[r * 6 + c] = JtJ[c * 6 + r] = sums[q++]; }
    for (int r = 0; r < 6; ++r) JtE[r] = sums[21 + r];
    if (n_accepted) *n_accepted = (int64_t)sums[27];
    return 0;
}

int pcr_get_trace(pcr_handle* h, int32_t* n_iters, double* JtJ, double* JtE, int64_t* n, double* x) {
    if (!h) return 1;
    if (!h->prm.record_trace) return fail(h, "trace not recorded: set pcr_params.record_trace");
    if (n_iters) *n_iters = h->loam.trace_iters;
    for (int i = 0; i < h->loam.trace_iters && i < (int)h->loam.trace_host.size(); ++i) {
        const LoamTrace& t = h->loam.trace_host[i];
        if (JtJ) memcpy(JtJ + i * 36, t.JtJ, sizeof(t.JtJ));
        if (JtE) memcpy(JtE + i * 6, t.JtE, sizeof(t.JtE));
        if (x) memcpy(x + i * 6, t.x, sizeof(t.x));
        if (n) n[i] = t.n;
    }
    return 0;
}

int pcr_get_trace_counts(pcr_handle* h, int64_t* cache_hits, int64_t* searches) {
    if (!h) return 1;
    if (!h->prm.record_trace) return fail(h, "trace not recorded: set pcr_params.record_trace");
    for (int i = 0; i < h->loam.trace_iters && i < (int)h->loam.trace_host.size(); ++i) {
        if (cache_hits) cache_hits[i] = h->loam.trace_host[i].cache_hits;
        if (searches) searches[i] = h->loam.trace_host[i].searches;
    }
    return 0;
}

int pcr_get_timeline(pcr_handle* h, uint64_t* out, size_t capacity, int* launches, int* blocks) {
    if (!h) return 1;
    if (h->prm.record_timeline != 1 || !h->loam.timeline.p) return fail(h, "timeline not recorded: set pcr_params.record_timeline = 1");
    const int nl = std::max(1, h->prm.loam_iters), nb = (int)h->loam.last_blocks;
    if (launches) *launches = nl;
    if (blocks) *blocks = nb;
    if (!out) return 0;
    if (capacity < (size_t)nl * nb * kTimelineSlots) return fail(h, "timeline buffer too small");
    H_TRY(hipStreamSynchronize(h->stream));
    for (int l = 0; l < nl; ++l)
        H_TRY(hipMemcpy(out + (size_t)l * nb * kTimelineSlots, h->loam.timeline.as<unsigned long long>() + (size_t)l * kMaxPartials * kTimelineSlots,
                        (size_t)nb * kTimelineSlots * sizeof(uint64_t),
                        hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
