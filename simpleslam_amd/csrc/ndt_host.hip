// ndt_host.hip -- NDT host driver: pclomp::NormalDistributionsTransform::computeTransformation
// (ndt_omp_impl.hpp:81-171) with the More-Thuente line search (:649-932).  pcr_ndt_derivatives and the pcr_ndt_opt_* entry points.

#include <algorithm>
#include <string>
#include <vector>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

// The base margin, in metres, of the region a target is prepared for (roi_enqueue): 1 m of translation + what the neighbourhood reaches beyond the
// cell a point lands in.  The region is a dilation by a CHEBYSHEV radius (grid_index.hip: every macro cell within r of a mark along x, then y,
// then z -- a box, not a ball), so the one voxel per axis that holds DIRECT7's face cells holds DIRECT26's edge and corner cells as well: no
// sqrt(3).  DIRECT1 keeps the voxel too: the mark pass places a point by floor(p / cell) in double and the lookup by floorf in float
// (ndt_neighbours), which may differ by a cell at a face; a smaller margin would need that bounded first.
static double ndt_roi_margin(int search, double res) {
    (void)search;      // PCR_NDT_DIRECT26, _DIRECT7, _DIRECT1: one voxel per axis in every case, for the reasons above
    return 1.0 + res;
}

// deferred: nothing is read back here -- the index is enqueued with the previous target's box as a hint and the cell table at its
// current size; whether either was wrong (header.overflow / header.stale) comes back with the result of the alignment
// (NdtOut), and the caller then prepares again the slow, checked way.  One host round trip less per scan.
int ndt_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, bool deferred, const RoiScan* roi_scan) {
    h->target_ready = false;
    h->roi_on = false;
    const double res = (double)(float)h->prm.ndt_resolution;     // resolution_ is a float (ndt_omp.h)
    if (!(res > 0)) return fail(h, "ndt_resolution must be positive");
    // the voxel lattice is VoxelGridCovariance's own (leaf index = floor(p * inverse_leaf) - min_b in float,
    // voxel_grid_covariance_omp_impl.hpp:218-220): GridHeader.pcl_mode, no pad cells
    h->grid.no_hints = h->prm.index_no_hints != 0;
    // prepared for one scan (pcr_scan2map): voxel Gaussians only where that scan can land (RoiView) -- and, when this build can take the
    // lattice and the tile layout of an earlier full build as they are, an index of the region's points only (BuildFilter)
    RoiView roi;
    memset(&roi, 0, sizeof roi);
    const bool want_roi = roi_scan && roi_scan->n_src > 0 && n_dst > 0;
    BuildFilter bf;
    bf.enqueue_mask = [&]() -> hipError_t {
        if (roi_enqueue(h, *roi_scan, res, ndt_roi_margin(h->prm.ndt_search, res), &roi)) return hipErrorUnknown;      // 1 m of translation + the neighbourhood's voxel, + 0.05 rad
        bf.mask = roi.mask; bf.mshift = roi.mshift;
        return hipSuccess;
    };
    // setMinPointPerVoxel (pclomp/voxel_grid_covariance_omp.h:229-240): "Covariance calculation requires at least 3 points"
    const int min_points = std::max(3, h->prm.ndt_min_points);
    const size_t max_vox = n_dst / (size_t)min_points + 2;      // a voxel needs min_points points
    H_TRY(h->nd.vox.reserve(max_vox * sizeof(NdtVoxel)));
    H_TRY(h->nd.list.reserve((max_vox + 64) * sizeof(uint32_t)));
    if (!h->nd.count.p) {      // two counters used alternately; each call leaves the other one cleared for the next (ndt_candidates_kernel)
        H_TRY(h->nd.count.reserve(256));
        H_TRY(hipMemsetAsync(h->nd.count.p, 0, 256, h->stream));
    }
    h->nd.count_idx ^= 1;
    uint32_t* const nd_count = h->nd.count.as<uint32_t>() + 32 * h->nd.count_idx;
    uint32_t* const nd_count_next = h->nd.count.as<uint32_t>() + 32 * (h->nd.count_idx ^ 1);
    if (deferred) {
        // (the cell table keeps its size in a deferred build, so the slots can be sized before it: a region-only build lists the voxel cells
        //  and writes the slots in its tile pass -- TileTail)
        if (h->grid.ensure_tables(h->stream, &h->err) != hipSuccess) return 1;
        H_TRY(h->nd.slot.reserve(((size_t)h->grid.cell_capacity + 64) * sizeof(uint32_t)));
        bf.want_tail = true;
        bf.tail.vox_slot = h->nd.slot.as<uint32_t>(); bf.tail.list = h->nd.list.as<uint32_t>(); bf.tail.count = nd_count; bf.tail.count_next = nd_count_next;
        bf.tail.min_points = min_points; bf.tail.capacity = (uint32_t)std::min<size_t>(max_vox, 0xffffffffu);
        const size_t cap_before = h->grid.cell_capacity;
        const void* const slot_before = h->nd.slot.p;
        if (h->grid.build(d_dst, n_dst, stride_floats, res, h->stream, &h->err, 0.0, 1, nullptr, true, want_roi ? &bf : nullptr) != hipSuccess) return 1;
        // (the tile pass has been handed vox_slot and the list BEFORE the build: nothing in build() may move them -- it never grows the cell table, only
        //  callers do -- but a change that broke that would write through a freed pointer: refuse loudly instead)
        if (bf.tail_applied && (h->grid.cell_capacity != cap_before || h->nd.slot.p != slot_before))
            return fail(h, "internal: the cell table changed size inside a deferred NDT build whose tile pass lists the voxel cells");
    } else if (settle_grid(h, h->grid, d_dst, n_dst, stride_floats, res, 1)) return 1;
    h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats; h->have_target = true;
    H_TRY(h->nd.slot.reserve(((size_t)h->grid.cell_capacity + 64) * sizeof(uint32_t)));
    if (bf.applied) { roi.filtered = 1; h->roi_on = true; }
    else if (want_roi) {
        if (roi_enqueue(h, *roi_scan, res, ndt_roi_margin(h->prm.ndt_search, res), &roi)) return 1;
        h->roi_on = true;
    }
    H_TRY(ndt_launch_voxels(h->grid, h->nd.slot.as<uint32_t>(), h->nd.vox.as<NdtVoxel>(), nd_count, nd_count_next, h->nd.list.as<uint32_t>(),
                            max_vox, min_points, 0.01, h->stream, h->roi_on ? &roi : nullptr, bf.tail_applied));
    h->target_ready = true;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

namespace ndt_host {
using namespace ndt_opt;      // pose_from_p, angle_derivatives, svd6_solve, the line search: shared with the device (ndt_opt.h)
// Matrix3f::eulerAngles(0, 1, 2)
void euler_xyz(const float R[9], float out[3]) {
    const float pi = 3.14159265358979323846f;
    float r0 = atan2f(R[1 * 3 + 2], R[2 * 3 + 2]);
    const float c2 = sqrtf(R[0] * R[0] + R[1] * R[1]);
    float r1;
    if (r0 > 0.f) { r0 -= pi; r1 = atan2f(-R[2], -c2); }
    else r1 = atan2f(-R[2], c2);
    const float s1 = sinf(r0), c1 = cosf(r0);
    const float r2 = atan2f(s1 * R[2 * 3 + 0] - c1 * R[1 * 3 + 0], c1 * R[1 * 3 + 1] - s1 * R[2 * 3 + 1]);
    out[0] = -r0; out[1] = -r1; out[2] = -r2;
}
}  // namespace ndt_host

// the guess as the optimiser starts from it: handed over as Matrix4f (NdtRegister.cpp:27), its Euler angles as the parameters
// (ndt_omp_impl.hpp:103-111)
void ndt_initial_pose(const double pose[16], NdtPose* T0, double p0[6]) {
    float G[16];
    for (int i = 0; i < 16; ++i) G[i] = (float)pose[i];
    for (int rr = 0; rr < 3; ++rr) { for (int c = 0; c < 3; ++c) T0->R[rr * 3 + c] = G[c * 4 + rr]; T0->t[rr] = G[12 + rr]; }
    float eul[3];
    ndt_host::euler_xyz(T0->R, eul);     // Transform::rotation() taken as the linear part
    p0[0] = T0->t[0]; p0[1] = T0->t[1]; p0[2] = T0->t[2]; p0[3] = eul[0]; p0[4] = eul[1]; p0[5] = eul[2];
}
// ... and the final transformation as the caller's pose
void ndt_pose_out(const NdtPose& T, double pose16[16]) {
    for (int i = 0; i < 16; ++i) pose16[i] = 0;
    for (int rr = 0; rr < 3; ++rr) { for (int c = 0; c < 3; ++c) pose16[c * 4 + rr] = (double)T.R[rr * 3 + c]; pose16[12 + rr] = (double)T.t[rr]; }
    pose16[15] = 1.0;
}

// The arguments of the handle's NDT launches over a source (run_ndt, pcr_ndt_derivatives): no region, no profiling counters
NdtArgs ndt_args(const pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats) {
    NdtArgs a;
    memset(&a, 0, sizeof a);
    a.src = d_src; a.n_src = (uint32_t)n_src; a.src_stride = (uint32_t)stride_floats;
    a.hdr = h->grid.header.as<GridHeader>(); a.vox_slot = h->nd.slot.as<uint32_t>(); a.vox = h->nd.vox.as<NdtVoxel>();
    a.partials = h->nd.partials.as<double>();
    a.use_tile = h->use_tile;
    a.search = h->prm.ndt_search;
    for (int d = 0; d < 3; ++d) { a.tile_lo[d] = h->tile_lo[d]; a.tile_hi[d] = h->tile_hi[d]; }
    // Gauss constants (ndt_omp_impl.hpp:86-93)
    const double res = (double)(float)h->prm.ndt_resolution;
    const double c1 = 10 * (1 - h->prm.ndt_outlier_ratio), c2 = h->prm.ndt_outlier_ratio / pow(res, 3), d3 = -log(c2);
    a.d1 = -log(c1 + c2) - d3;
    a.d2 = -2 * log((-log(c1 * exp(-0.5) + c2) - d3) / a.d1);
    return a;
}

// One evaluation pass of the host-driven loop: the kernel `kind` names at pose T, the fold, the ranks' sum.
int ndt_host_pass(pcr_handle* h, const NdtArgs& a, int kind, const NdtPose& T, const NdtAngles& ang, double sums[43]) {
    h->seq += 1.0;
    if (kind == kNdtPassHessian) H_TRY(ndt_launch_hessian(a, T, ang, h->nd.out48.dev, h->stream, h->seq));
    else H_TRY(ndt_launch_derivatives(a, T, ang, kind == kNdtPassDerivH ? 1 : 0, h->nd.out48.dev, h->stream, h->seq));
    if (wait_result(h, &h->nd.out48.host[47], h->seq)) return 1;
    if (sharded(h) && ranks_allreduce(h, h->nd.out48.host, 43)) return 1;      // score, gradient, Hessian summed over the ranks' tiles
    for (int i = 0; i < 43; ++i) sums[i] = h->nd.out48.host[i];
    return 0;
}

// computeDerivatives (with the Hessian) at parameters p with the cloud transformed by T: the 43 sums, and the angle tables of p
int ndt_derivatives(pcr_handle* h, const NdtArgs& a, const NdtPose& T, const double p[6], NdtAngles* ang, double sums[43]) {
    ndt_host::angle_derivatives(p, ang);
    memset(sums, 0, 43 * sizeof(double));      // (an empty scan sums nothing)
    if (a.n_src == 0) return 0;
    ++h->nd.deriv;
    return ndt_host_pass(h, a, kNdtPassDerivH, T, *ang, sums);
}

}  // namespace

namespace pcr {
namespace host {

// pcr_scan2map, a target prepared for the scan's region: the optimiser's initial state at `pose` made a rider of the launch that marks
// the region (roi_enqueue launches h->blob; run_ndt then starts without a launch for it)
int ndt_ride_initial_state(pcr_handle* h, const double pose[16]) {
    NdtPose T0;
    double p0[6];
    ndt_initial_pose(pose, &T0, p0);
    H_TRY(h->nd.ctl.reserve(2 * sizeof(NdtCtl)));
    ndt_ctl_init_blob(&h->blob, h->nd.ctl.as<NdtCtl>(), T0, p0, h->prm.ndt_step_size, h->prm.ndt_trans_eps, h->prm.ndt_max_iters, h->prm.ndt_evaluate_repeats);
    h->blob_pending = true;
    return 0;
}

// Each of run_ndt's three loops hands the driver an NdtOut: a device loop the one it reported in, the host loop what it has of it (pose,
// verdict, counters).  bail: a device loop met a (nearly) singular Newton system and the host loop decides, with the SVD.
static constexpr const char *kNdtWindowMsg = "ndt_max_iters exceeds the device loop's pass window (2^20 passes)",
                            *kNdtBudgetMsg = "ndt: the optimiser did not finish within its pass budget";

// The device-resident loop of an unsharded handle: one launch per pass (ndt.hip: ndt_pass_pro_kernel), enqueued ahead of the device while
// the host watches a progress word.
static int ndt_loop_device(pcr_handle* h, const NdtArgs& a, const NdtPose& T0, const double p0[6], NdtOut* res) {
    NdtCtl* d_ctl = h->nd.ctl.as<NdtCtl>();
    NdtOut* out = h->nd.out.host;
    const double seq = (h->seq += 1.0);
    // (a scan2map call whose region was marked has stored this state with the mark pass: ndt_scan2map, BlobStore)
    const bool stored = h->blob_stored && h->roi_on;
    h->blob_stored = false;
    if (!stored) H_TRY(ndt_launch_ctl_init(d_ctl, T0, p0, h->prm.ndt_step_size, h->prm.ndt_trans_eps, h->prm.ndt_max_iters, h->stream, h->prm.ndt_evaluate_repeats,
                                           a.roi_escapes));
    const int limit = (h->prm.ndt_max_iters + 3) * 13 + 5;        // an iteration takes at most 1 + 10 + 1 passes; one launch more finishes
    auto launch = [&](long i) -> hipError_t {
        const int index = (int)i;
        hipEvent_t ev[2] = {nullptr, nullptr};
        if (h->profile >= 2) {      // events at every launch's own begin and end (pcr_stats.kernel_ms)
            while ((int)h->ev_kernel.size() < 2 * (index + 1)) { hipEvent_t e; hipError_t er = hipEventCreate(&e); if (er != hipSuccess) return er; h->ev_kernel.push_back(e); }
            h->nd_prof_launches = index + 1; ev[0] = h->ev_kernel[2 * index]; ev[1] = h->ev_kernel[2 * index + 1];
        }
        return ndt_launch_pass_pro(a, d_ctl, h->nd.partials.as<double>(), h->nd.out.dev, h->stream, seq, index, ev[0], ev[1]);
    };
    // (the host enqueues a pass in a quarter of the time the device needs for one: it only has to stay two ahead -- a pass enqueued beyond
    //  the end costs ~10 us of device time)
    static constexpr PaceRule kRule{3, 2, 4, false};
    if (pace_passes(h, out, seq, limit, kRule, kNdtWindowMsg, kNdtBudgetMsg, launch)) return 1;
    *res = *out;
    return 0;
}

// The device-resident loop of a sharded handle, two launches per pass or three: over the peer exchange (pcr_comm_init_peer) the evaluation, then
// fold + exchange + controller step in one (ndt.hip: ndt_fold_exchange_ctl_kernel), paced like the unsharded loop; over RCCL fold -> ncclAllReduce
// on the handle's stream -> controller step, in batches of a fixed number of passes -- whether another batch is due is decided from the
// controller state the ranks share, so every rank enqueues the same collectives.  (A host-supplied collective needs the host in every
// pass: the host loop.)
static int ndt_loop_device_sharded(pcr_handle* h, const NdtArgs& a, const NdtPose& T0, const double p0[6], NdtOut* res) {
    NdtCtl* d_ctl = h->nd.ctl.as<NdtCtl>();
    NdtOut* out = h->nd.out.host;
    H_TRY(h->nd.sums.reserve(64 * sizeof(double)));
    const double seq = (h->seq += 1.0);
    H_TRY(ndt_launch_ctl_init(d_ctl, T0, p0, h->prm.ndt_step_size, h->prm.ndt_trans_eps, h->prm.ndt_max_iters, h->stream, h->prm.ndt_evaluate_repeats));
    const int limit = (h->prm.ndt_max_iters + 3) * 13 + 4, kBatch = 6;
    if (h->comm.peer_on) {
        // passes are queued a fixed number ahead of the progress word, one at a time -- by the rule that leaves every rank with the same number of
        // launches queued (PaceRule::peer): the ranks' sequence numbers, one per launch, agree in the next call too.
        auto launch = [&](long) -> hipError_t { h->comm.peer_seq += 1.0; return ndt_launch_pass_peer(a, d_ctl, h->comm.peer, h->comm.peer_seq, h->nd.out.dev, h->stream, seq); };
        if (pace_passes(h, out, seq, limit, kPeerPace, kNdtWindowMsg, kNdtBudgetMsg, launch)) return 1;
    } else {
        const volatile double* f_batch = &out->batch;
        for (int batch = 1, enq = 0;; ++batch) {
            for (int b = 0; b < kBatch; ++b, ++enq) {
                H_TRY(ndt_launch_pass_fold(a, d_ctl, h->nd.sums.as<double>(), h->stream));      // (a rank with an empty scan still folds zeros and takes part)
                if (rccl_sum(h, h->nd.sums.p, 48)) return 1;
                H_TRY(ndt_launch_ctl(a, d_ctl, h->nd.sums.as<double>(), h->nd.out.dev, h->stream, seq, b == kBatch - 1 ? batch : 0));
            }
            const double want0 = seq * 65536.0 + 2.0 * batch;
            long spins = 0;
            while (!(*f_batch == want0 || *f_batch == want0 + 1.0)) {
                __builtin_ia32_pause();
                if (++spins > 400000 || h->profile != 0) { H_TRY(hipStreamSynchronize(h->stream)); if (!(*f_batch == want0 || *f_batch == want0 + 1.0)) return fail(h, "ndt: the sharded device loop lost its batch marker"); }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (peer_check(h)) return 1;      // (an exchange of this batch timed out: the loop has stopped on the ranks that waited, the session is over)
            if (*f_batch == want0 + 1.0) break;
            if (enq >= limit) return fail(h, kNdtBudgetMsg);
        }
    }
    *res = *out;      // (bail: every rank saw the same pivots and goes to the host loop)
    return 0;
}

// The host-driven loop: the state machine on the host (with the SVD), one round trip per pass; sharded, every pass's sums cross the ranks.
static int ndt_loop_host(pcr_handle* h, const NdtArgs& a, const NdtPose& T0, const double p0[6], NdtOut* res) {
    NdtCtl c;
    ndt_opt::ctl_init(&c, T0, p0, h->prm.ndt_step_size, h->prm.ndt_trans_eps, h->prm.ndt_max_iters);
    c.replay_off = h->prm.ndt_evaluate_repeats ? 1 : 0;
    double sums[43];
    while (!c.done) {
        if (a.n_src == 0) memset(sums, 0, sizeof sums);        // an empty scan: computeDerivatives sums nothing
        else if (ndt_host_pass(h, a, c.kind, c.T, c.ang, sums)) return 1;
        ndt_opt::ctl_step(&c, sums);
    }
    memset(res, 0, sizeof *res);
    res->final_T = c.final_T; res->score = c.score; res->conv = c.conv; res->nr_it = c.nr_it; res->n_deriv = c.n_deriv; res->n_hess = c.n_hess; res->passes = c.passes;
    return 0;
}

// Returns 0 with nd_grid_bad set when the index must be prepared again and the call repeated, 2 when a target prepared for the scan's
// region has to give way to the whole target.
int run_ndt(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) {
    if (!h->target_ready) return fail(h, "no target prepared");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    H_TRY(h->nd.out48.ensure(48));
    H_TRY(h->nd.out.ensure());
    H_TRY(h->nd.partials.reserve((size_t)1024 * 48 * sizeof(double)));      // (one buffer of 1024 rows, or the two of 256 of the one-launch-per-pass loop)
    H_TRY(h->nd.ctl.reserve(2 * sizeof(NdtCtl)));
    NdtArgs a = ndt_args(h, d_src, n_src, stride_floats);
    a.roi_escapes = roi_view(h).escapes;      // (nullptr unless the target was prepared for one scan)
    a.pair_count = prof_counters(h);
    h->nd.iters = h->nd.deriv = h->nd.hess = 0;
    NdtPose T0;
    double p0[6];
    ndt_initial_pose(pose, &T0, p0);

    // The loop stays on the device unless pcr_params.host_optimiser asks for the host loop, the scan is empty, or the sums of a sharded
    // handle cross the ranks through the host (pcr_comm_init_host).
    const bool dev_sharded = sharded(h) && (h->comm.rccl || h->comm.peer_on) && !h->comm.host_ar && n_src > 0 && h->prm.host_optimiser == 0;
    const bool on_device = n_src > 0 && !sharded(h) && h->prm.host_optimiser == 0;
    if (h->roi_on && !on_device) return fail(h, "internal: a target prepared for one scan needs the device-resident loop");
    h->nd_grid_checked = false; h->nd_grid_bad = false;
    NdtOut res;
    bool device_loop = false;      // res is a device loop's: it did not bail
    if (dev_sharded) {
        if (ndt_loop_device_sharded(h, a, T0, p0, &res)) return 1;
        device_loop = !res.bail;
    } else if (on_device) {
        if (ndt_loop_device(h, a, T0, p0, &res)) return 1;
        h->nd_grid_bad = res.grid_overflow || res.grid_stale;      // (what the loop saw in the index header: ndt_scan2map reads it)
        h->nd_grid_empty = res.grid_empty != 0; h->nd_grid_cells = res.grid_cells; h->nd_grid_checked = true;
        if (h->nd_grid_bad) return 0;           // the caller prepares the target again and repeats the call
        // a pass looked up a voxel the target was not prepared for (RoiView), or the loop wants the host's SVD: whole target, again
        if (h->roi_on && (res.roi_escapes > 0 || res.bail)) { h->roi_repeats += 1; return 2; }
        device_loop = !res.bail;
    }
    if (!device_loop && ndt_loop_host(h, a, T0, p0, &res)) return 1;
    ndt_pose_out(res.final_T, pose);
    if (converged) *converged = res.conv ? 1 : 0;
    h->nd.iters = res.nr_it; h->nd.score = res.score; h->nd.deriv = res.n_deriv; h->nd.hess = res.n_hess;
    h->stats.iterations = res.nr_it; h->stats.kernel_launches = res.n_deriv + res.n_hess;
    h->stats.attempts = device_loop ? res.passes : 0;      // (the passes a device loop actually evaluated; 0: not such a loop)
    h->stats.n_src = (int64_t)n_src; h->stats.n_dst = (int64_t)h->tgt_n;
    return 0;
}

// ---- ndt's row of the method table (handle.h: MethodOps; its align is run_ndt) ----
int ndt_scan2map(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged) {
    // NdtRegister::scan2Map calls setInputTarget every time, which rebuilds the voxel grid (NdtRegister.cpp:23)
    // Unsharded: the index is enqueued unchecked (previous box as a hint, cell table as it is) and the alignment's own result
    // says whether that held; if not, once more with the checked build.
    const bool try_deferred = !sharded(h) && n_src > 0 && h->prm.host_optimiser == 0;
    double pose_in[16];
    memcpy(pose_in, pose, sizeof pose_in);
    // (unsharded, device loop: the voxel Gaussians are prepared only where this scan can land -- RoiView; a call that leaves the
    //  region is repeated on the whole target)
    bool use_roi = try_deferred && h->prm.full_target == 0;
    const RoiScan rs{d_src, n_src, stride_floats, pose_in};
    for (int attempt = 0; attempt < 3; ++attempt) {
        const bool deferred = try_deferred && attempt == 0;
        h->blob_pending = h->blob_stored = false;
        // the optimiser's initial state rides on the launch that marks the region (run_ndt then starts without a launch for it)
        if (use_roi && ndt_ride_initial_state(h, pose)) return 1;
        const int prep_rc = ndt_prepare_target(h, d_dst, n_dst, stride_floats, deferred, use_roi ? &rs : nullptr);
        h->blob_pending = false;
        if (agree_prepared(h, prep_rc)) { h->blob_stored = false; return 1; }
        if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_index, h->stream));
        const int rrc = run_ndt(h, d_src, n_src, stride_floats, pose, converged);
        h->blob_stored = false;
        if (rrc == 2) { use_roi = false; memcpy(pose, pose_in, sizeof pose_in); if (deferred && h->nd_grid_checked && !h->nd_grid_bad && !h->nd_grid_empty) { h->grid.confirm(); h->grid.note_cells(h->nd_grid_cells); } continue; }
        if (rrc) return 1;
        if (!deferred) break;
        if (h->nd_grid_checked && !h->nd_grid_bad) { if (!h->nd_grid_empty) { h->grid.confirm(); h->grid.note_cells(h->nd_grid_cells); } break; }
        // the hint or the table size did not hold (or the device loop handed over to the host before it could tell): checked build
        h->grid.hint_margin = 8; h->grid.cells_hint = 0;      // (a cloud that left the old box: its cell count is anybody's guess too)
        memcpy(pose, pose_in, sizeof pose_in);
    }
    return end_timed_call(h);
}
int ndt_kept_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) { return agree_prepared(h, ndt_prepare_target(h, d_dst, n_dst, stride_floats)); }
// the voxel Gaussians: the lattice's cell and the points a voxel needs
bool ndt_target_from_changed(const pcr_params& old_p, const pcr_params& new_p) { return new_p.ndt_resolution != old_p.ndt_resolution || new_p.ndt_min_points != old_p.ndt_min_points; }

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_ndt_derivatives(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double p[6],
                        double* score, double grad[6], double hess[36], double* hess_d) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kNdt) return fail(h, "pcr_ndt_derivatives needs an ndt handle");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->target_ready) return fail(h, "no target: call pcr_set_target first");
    if (ensure_full_target(h)) return 1;
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    H_TRY(h->nd.out48.ensure(48));
    H_TRY(h->nd.partials.reserve((size_t)1024 * 48 * sizeof(double)));
    const NdtArgs a = ndt_args(h, d_src, n_src, stride_bytes / 4);
    NdtPose T;
    NdtAngles ang;
    ndt_host::pose_from_p(p, &T);
    double sums[43];
    if (ndt_derivatives(h, a, T, p, &ang, sums)) return 1;
    if (score) *score = sums[0];
    memcpy(grad, sums + 1, 6 * sizeof(double)); memcpy(hess, sums + 7, 36 * sizeof(double));
    if (hess_d && n_src) {      // computeHessian at the same pose
        if (ndt_host_pass(h, a, kNdtPassHessian, T, ang, sums)) return 1;
        memcpy(hess_d, sums + 7, 36 * sizeof(double));
    }
    return 0;
}

/* ---- read-only introspection for the test suite: nothing below is called by pcr_scan2map / pcr_align ---- */

int pcr_ndt_voxels(pcr_handle* h, pcr_ndt_voxel* out, size_t capacity, size_t* count, size_t* rejected) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kNdt) return fail(h, "pcr_ndt_voxels needs an ndt handle");
    if (set_device(h)) return 1;
    if (!h->target_ready) return fail(h, "no target: call pcr_set_target first");
    if (h->roi_on) return fail(h, "pcr_ndt_voxels: pcr_scan2map prepared this target for that one scan's region only; call pcr_set_target for a target that is kept");
    H_TRY(hipStreamSynchronize(h->stream));
    GridHeader hd;
    H_TRY(hipMemcpy(&hd, h->grid.header.p, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.overflow || hd.stale) return fail(h, "internal: the index of a target that pcr_set_target settled is incomplete");
    size_t n_list = 0;
    if (!hd.empty) {
        // (the list's length: the counter this target's candidates pass counted in, capped like ndt_voxel_kernel caps it)
        uint32_t cnt = 0;
        H_TRY(hipMemcpy(&cnt, h->nd.count.as<uint32_t>() + 32 * h->nd.count_idx, sizeof cnt, hipMemcpyDeviceToHost));
        const size_t max_vox = h->tgt_n / (size_t)std::max(3, h->prm.ndt_min_points) + 2;
        n_list = std::min<size_t>(cnt, max_vox);
    }
    std::vector<uint32_t> list(n_list), slot(n_list ? (size_t)hd.n_cells : 0);
    std::vector<NdtVoxel> vox(n_list);
    if (n_list) {
        H_TRY(hipMemcpy(list.data(), h->nd.list.p, n_list * sizeof(uint32_t), hipMemcpyDeviceToHost));
        H_TRY(hipMemcpy(slot.data(), h->nd.slot.p, slot.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        H_TRY(hipMemcpy(vox.data(), h->nd.vox.p, n_list * sizeof(NdtVoxel), hipMemcpyDeviceToHost));
    }
    size_t kept = 0;
    for (size_t li = 0; li < n_list; ++li) {
        const uint32_t t = list[li];
        if (t >= slot.size()) return fail(h, "internal: a listed NDT cell lies outside the lattice");
        if (slot[t] != (uint32_t)li + 1u) continue;      // rejected by the eigenvalue or the inverse test: the slot stayed 0
        if (out && kept < capacity) {
            const uint32_t d0 = (uint32_t)hd.dims[0], d1 = (uint32_t)hd.dims[1], row = t / d0, cz = row / d1;
            pcr_ndt_voxel& o = out[kept];
            // the lattice coordinate floorf(p * inv_leaf): the cell's position in the box + min_b (org holds the same number)
            o.ijk[0] = (int32_t)(t - row * d0) + (int32_t)hd.org[0]; o.ijk[1] = (int32_t)(row - cz * d1) + (int32_t)hd.org[1]; o.ijk[2] = (int32_t)cz + (int32_t)hd.org[2];
            o.n = vox[li].n;
            memcpy(o.mean, vox[li].mean, sizeof o.mean);
            memcpy(o.icov, vox[li].icov, sizeof o.icov);
        }
        ++kept;
    }
    if (count) *count = kept;
    if (rejected) *rejected = n_list - kept;
    if (out && capacity < kept) return fail(h, "pcr_ndt_voxels: room for " + std::to_string(capacity) + " voxels, the target has " + std::to_string(kept));
    return 0;
}

int pcr_ndt_pass_sums(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double p[6], int kind,
                      double* score, double grad[6], double hess[36]) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kNdt) return fail(h, "pcr_ndt_pass_sums needs an ndt handle");
    if (kind != kNdtPassDerivH && kind != kNdtPassDeriv && kind != kNdtPassHessian) return fail(h, "pcr_ndt_pass_sums: kind must be 0, 1 or 2");
    if (!p || !grad || !hess) return fail(h, "pcr_ndt_pass_sums: p, grad or hess is NULL");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->target_ready) return fail(h, "no target: call pcr_set_target first");
    if (sharded(h)) return fail(h, "pcr_ndt_pass_sums: a handle with a communicator does not run the one-launch-per-pass loop");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    if (ensure_full_target(h)) return 1;
    if (score) *score = 0;
    memset(grad, 0, 6 * sizeof(double)); memset(hess, 0, 36 * sizeof(double));
    if (n_src == 0) return 0;      // (run_ndt does not start the device loop on an empty scan either)
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    H_TRY(h->nd.out.ensure());
    H_TRY(h->nd.partials.reserve((size_t)1024 * 48 * sizeof(double)));
    H_TRY(h->nd.ctl.reserve(2 * sizeof(NdtCtl)));
    const NdtArgs a = ndt_args(h, d_src, n_src, stride_bytes / 4);
    // A state that asks for ONE pass of `kind` at p and for nothing after it: the pass is taken as the evaluation that ends a line search
    // of step 0 in an iteration past max_iters, so ctl_decide takes the sums in (score and gradient, or the Hessian), finds the loop
    // converged and leaves them in the state it hands on.
    NdtCtl c;
    memset(&c, 0, sizeof c);
    NdtPose T;
    ndt_host::pose_from_p(p, &T);
    ndt_opt::ctl_init(&c, T, p, 0.1, 1.0, 0);
    c.kind = kind; c.phase = kNdtPhaseLsHess; c.nr_it = 1; c.a_t = 0.0;
    NdtCtl* const d_ctl = h->nd.ctl.as<NdtCtl>();
    const double seq = (h->seq += 1.0);
    H_TRY(ndt_launch_ctl_state(d_ctl, c, h->stream));
    H_TRY(ndt_launch_pass_pro(a, d_ctl, h->nd.partials.as<double>(), h->nd.out.dev, h->stream, seq, 0));      // the pass
    H_TRY(ndt_launch_pass_pro(a, d_ctl, h->nd.partials.as<double>(), h->nd.out.dev, h->stream, seq, 1));      // its prologue folds the rows and decides
    H_TRY(hipMemcpyAsync(&c, d_ctl + 1, sizeof c, hipMemcpyDeviceToHost, h->stream));
    H_TRY(hipStreamSynchronize(h->stream));
    if (h->nd.out.host->seq != seq || !c.done || c.bail || c.passes != 1) return fail(h, "internal: pcr_ndt_pass_sums: the loop did not end after its one pass");
    if (score) *score = c.score;
    for (int i = 0; i < 6; ++i) grad[i] = c.grad[i];
    for (int i = 0; i < 36; ++i) hess[i] = c.hess[i];
    return 0;
}

// d_*: a device object (pcr_ndt_opt_create_device): the state lives in device memory and every feed is one launch of ndt_ctl_kernel, the
// controller step of the sharded device loop; `c` is then the copy that launch left behind.  All NULL: the host's ctl_step.
struct pcr_ndt_opt { NdtCtl c; NdtCtl* d_ctl; double* d_sums; GridHeader* d_hdr; NdtOut* d_out; };

static pcr_ndt_opt* ndt_opt_new(const double pose_guess[16], double step_size, double trans_eps, int max_iters) {
    if (!pose_guess) return nullptr;
    pcr_ndt_opt* o = new pcr_ndt_opt;
    memset(o, 0, sizeof *o);
    NdtPose T0;
    double p0[6];
    ndt_initial_pose(pose_guess, &T0, p0);      // (as run_ndt starts)
    ndt_opt::ctl_init(&o->c, T0, p0, step_size, trans_eps, max_iters);
    return o;
}
pcr_ndt_opt* pcr_ndt_opt_create(const double pose_guess[16], double step_size, double trans_eps, int max_iters) {
    return ndt_opt_new(pose_guess, step_size, trans_eps, max_iters);
}
pcr_ndt_opt* pcr_ndt_opt_create_device(const double pose_guess[16], double step_size, double trans_eps, int max_iters) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return nullptr; }
    pcr_ndt_opt* o = ndt_opt_new(pose_guess, step_size, trans_eps, max_iters);
    if (!o) return nullptr;
    const bool ok = hipMalloc(&o->d_ctl, sizeof(NdtCtl)) == hipSuccess && hipMalloc(&o->d_sums, 48 * sizeof(double)) == hipSuccess &&
                    hipMalloc(&o->d_hdr, sizeof(GridHeader)) == hipSuccess && hipMalloc(&o->d_out, sizeof(NdtOut)) == hipSuccess &&
                    hipMemset(o->d_sums, 0, 48 * sizeof(double)) == hipSuccess && hipMemset(o->d_hdr, 0, sizeof(GridHeader)) == hipSuccess &&
                    hipMemset(o->d_out, 0, sizeof(NdtOut)) == hipSuccess && ndt_launch_ctl_state(o->d_ctl, o->c, nullptr) == hipSuccess &&
                    hipDeviceSynchronize() == hipSuccess;
    if (!ok) { pcr_ndt_opt_destroy(o); return nullptr; }
    return o;
}
void pcr_ndt_opt_destroy(pcr_ndt_opt* o) {
    if (!o) return;
    if (o->d_ctl) (void)hipFree(o->d_ctl);
    if (o->d_sums) (void)hipFree(o->d_sums);
    if (o->d_hdr) (void)hipFree(o->d_hdr);
    if (o->d_out) (void)hipFree(o->d_out);
    delete o;
}
int pcr_ndt_opt_set_replay(pcr_ndt_opt* o, int off) {
    if (!o || o->c.passes || o->c.done) return 1;      // (before the first feed)
    o->c.replay_off = off ? 1 : 0;
    if (o->d_ctl && (ndt_launch_ctl_state(o->d_ctl, o->c, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) return 1;
    return 0;
}
int pcr_ndt_opt_request(const pcr_ndt_opt* o, int* kind, double p6[6], double pose16[16]) {
    if (!o || !kind) return 1;
    *kind = o->c.done ? kNdtPassNone : o->c.kind;
    if (p6) for (int i = 0; i < 6; ++i) p6[i] = o->c.x_t[i];
    if (pose16) ndt_pose_out(o->c.T, pose16);
    return 0;
}
int pcr_ndt_opt_feed(pcr_ndt_opt* o, const double sums[43]) {
    if (!o || !sums || o->c.done) return 1;
    if (!o->d_ctl) { ndt_opt::ctl_step(&o->c, sums); return 0; }
    double s48[48];
    for (int i = 0; i < 48; ++i) s48[i] = i < 43 ? sums[i] : 0.0;
    NdtArgs a;
    memset(&a, 0, sizeof a);
    a.hdr = o->d_hdr;
    // (a step that fails half-way may have moved the device's state past the copy here: the object ends, handed back like a bail)
    const bool ok = hipMemcpy(o->d_sums, s48, sizeof s48, hipMemcpyHostToDevice) == hipSuccess &&
                    ndt_launch_ctl(a, o->d_ctl, o->d_sums, o->d_out, nullptr, 1.0, 0) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(&o->c, o->d_ctl, sizeof o->c, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) { o->c.done = 1; o->c.conv = 0; o->c.bail = 1; o->c.kind = kNdtPassNone; return 1; }
    return 0;
}
int pcr_ndt_opt_state(const pcr_ndt_opt* o, int* bail, int* late_h, double* a_t, int* phase) {
    if (!o) return 1;
    if (bail) *bail = o->c.bail;
    if (late_h) *late_h = o->c.late_h;
    if (a_t) *a_t = o->c.a_t;
    if (phase) *phase = o->c.phase;
    return 0;
}
int pcr_ndt_opt_tables(const pcr_ndt_opt* o, float j[24], float h[45], double jd[24], double hd[45]) {
    if (!o) return 1;
    if (j) memcpy(j, o->c.ang.j, sizeof o->c.ang.j);
    if (h) memcpy(h, o->c.ang.h, sizeof o->c.ang.h);
    if (jd) memcpy(jd, o->c.ang.jd, sizeof o->c.ang.jd);
    if (hd) memcpy(hd, o->c.ang.hd, sizeof o->c.ang.hd);
    return 0;
}
int pcr_ndt_opt_hessian(const pcr_ndt_opt* o, double hess[36]) {
    if (!o || !hess) return 1;
    for (int i = 0; i < 36; ++i) hess[i] = o->c.hess[i];
    return 0;
}
int pcr_ndt_opt_result(const pcr_ndt_opt* o, double pose16[16], int* converged, int* iterations, int* done) {
    if (!o) return 1;
    if (pose16) ndt_pose_out(o->c.final_T, pose16);
    if (converged) *converged = o->c.conv;
    if (iterations) *iterations = o->c.nr_it;
    if (done) *done = o->c.done;
    return 0;
}

int pcr_ndt_opt_counts(const pcr_ndt_opt* o, int* evaluations, int* hessians, int* replayed) {
    if (!o) return 1;
    if (evaluations) *evaluations = o->c.n_deriv;
    if (hessians) *hessians = o->c.n_hess;
    if (replayed) *replayed = o->c.replayed;
    return 0;
}

}  // extern "C"
