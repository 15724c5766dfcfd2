// gicp_host.hip -- GICP's host side: fast_gicp::FastGICP (fast_gicp_impl.hpp:103-237), the preparation of its target, its refusals and
// pcr_gicp_linearize.  PCL's align() and the LsqRegistration loop around its passes are lsq_host.h's run_lsq, the driver VGICP runs too; the
// scan's side is VGICP's (vgicp_host.hip: vgicp_source_enqueue / vgicp_source_settle).

#include <algorithm>

#include "lsq_host.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

// The whole target, always: an index of every finite point for the exact 1-NN (h->grid, with the coarse level of a scan-sized cloud's
// covariance search in h->cov_l1) and the covariance of every point.  A box no dense table can hold would need a cut index: refused.
int gicp_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, const std::function<int()>* before_wait) {
    h->target_ready = false;
    h->roi_on = false;
    h->clamp.use = 0;
    const double res = h->prm.vgicp_resolution;
    if (!(res > 0)) return fail(h, "gicp: vgicp_resolution (the cell of the target index) must be positive");
    if (h->prm.vgicp_k_corr != 20) return fail(h, "gicp: this build supports vgicp_k_corr = 20 (the reference's value) only");
    if (sharded(h) || h->use_tile) return fail(h, "gicp: sharded targets are not supported in this version");
    if (n_dst > kMaxPoints) return fail(h, "gicp: target cloud too large");
    // Every pass reads b_j at its original index, so the points must live as long as the prepared target does: a device buffer of the
    // caller's (pcr_scan2map_device, a sub-map) is copied into the handle's own staging area first, where pcr_set_target and the host
    // entry points have put theirs already.  Index, covariances and passes all read that copy.
    if (n_dst > 0 && d_dst != h->tgt_stage.as<float>()) {
        const size_t bytes = n_dst * stride_floats * sizeof(float);
        H_TRY(h->tgt_stage.reserve(bytes));
        H_TRY(hipMemcpyAsync(h->tgt_stage.p, d_dst, bytes, hipMemcpyDeviceToDevice, h->stream));
        d_dst = h->tgt_stage.as<float>();
    }
    h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats;
    H_TRY(h->gi.tgt_cov6.reserve((n_dst + 1) * 6 * sizeof(double)));
    CovSettle opt;
    bool untabulatable = false;
    opt.hdr0_out = &h->vg.cov_hdr0; opt.before_wait = before_wait; opt.untabulatable = &untabulatable;
    if (settle_cov_levels(h, h->grid, h->cov_l1, h->vg.cov_l2, d_dst, n_dst, stride_floats, res, opt)) {
        h->err = untabulatable ? "gicp: the target's box cannot be tabulated (" + h->err + "; a stray point far from the map?): that needs a cut index, which gicp "
                                 "does not support in this version"
                               : "gicp: preparing the target: " + h->err;
        return 1;
    }
    h->have_target = true;
    const int levels = cov_levels(n_dst);
    const GridIndex* cov_grid = &h->grid;
    h->cov_scale_hint = 0.0;
    if (const double scale = cov_search_scale(h->vg.cov_hdr0, n_dst); scale > 0.0) {      // (a map-sized cloud: one level, of a cell of its own)
        if (settle_grid(h, h->cov_l1, d_dst, n_dst, stride_floats, res * scale, 0, nullptr)) return fail(h, "gicp: preparing the target: " + h->err);
        h->cov_scale_hint = scale;
        cov_grid = &h->cov_l1;
    }
    H_TRY(vgicp_launch_cov(*cov_grid, levels > 1 ? &h->cov_l1 : nullptr, levels > 2 ? &h->vg.cov_l2 : nullptr, d_dst, stride_floats, n_dst,
                           h->gi.tgt_cov6.as<double>(), h->stream, h->prm.vgicp_regularization, nullptr, nullptr, &h->vg.tgt_scratch));
    h->target_ready = true;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

// the gate as the reference forms it: a float product (fast_gicp_impl.hpp:136); (float)FLT_MAX squared is +inf
float gicp_thr2(const pcr_handle* h) {
    const volatile float d = (float)h->prm.gicp_max_corr_dist;
    return d * d;
}

// The arguments of the handle's GICP launches over a source
GicpArgs gicp_args(const pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats) {
    GicpArgs a;
    memset(&a, 0, sizeof a);
    a.src = d_src; a.n_src = (uint32_t)n_src; a.src_stride = (uint32_t)stride_floats;
    a.src_cov6 = h->vg.src_cov6.as<double>();
    a.grid = h->grid.view();
    a.tgt = h->tgt_ptr; a.tgt_stride = (uint32_t)h->tgt_stride;
    a.tgt_cov6 = h->gi.tgt_cov6.as<double>();
    a.corr = h->gi.corr[0].as<uint32_t>(); a.corr_M = h->gi.M[0].as<double>();
    a.corr_next = h->gi.corr[1].as<uint32_t>(); a.corr_M_next = h->gi.M[1].as<double>();
    a.partials = h->vg_partials.as<double>();
    a.thr2 = gicp_thr2(h);
    return a;
}

// the scan's covariances settled, the correspondence buffers and the rows' memory in place
int gicp_setup(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats) {
    if (!h->target_ready) return fail(h, "no target prepared");
    if (sharded(h) || h->use_tile) return fail(h, "gicp: sharded handles are not supported in this version");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    if (ensure_out32(h)) return 1;
    if (vgicp_source_settle(h, d_src, n_src, stride_floats)) return 1;
    for (int k = 0; k < 2; ++k) {
        H_TRY(h->gi.corr[k].reserve((n_src + 1) * sizeof(uint32_t)));
        H_TRY(h->gi.M[k].reserve((n_src + 1) * 6 * sizeof(double)));
    }
    H_TRY(h->vg_partials.reserve((size_t)2 * 512 * 32 * sizeof(double)));
    return 0;
}

}  // namespace

namespace pcr {
namespace host {

int run_gicp(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) {
    const bool kept = fitness_scan_kept(h, d_src);
    if (gicp_setup(h, d_src, n_src, stride_floats)) return 1;
    if (keep_scan_for_fitness(h, d_src, n_src, stride_floats, kept)) return 1;
    const GicpArgs a = gicp_args(h, d_src, n_src, stride_floats);
    const bool on_device = n_src > 0 && h->prm.host_optimiser == 0 && h->prm.vgicp_max_iters > 0;
    auto device_pass = [&](long i, VgCtl* d_ctl, VgOut* d_out, double seq) { return gicp_launch_pass_pro(a, d_ctl, h->vg_partials.as<double>(), d_out, h->stream, seq, (int)i); };
    auto host_pass = [&](int kind, int parity, const Pose16& xi, double seq) {
        return (kind == kVgPassLinearize ? gicp_launch_linearize : gicp_launch_error)(swapped(a, parity), xi, h->out32.dev, h->stream, seq);
    };
    LsqResult r;
    if (run_lsq(h, pose, on_device, kLsqPace, "gicp: the optimiser did not finish within its pass budget", device_pass, host_pass, &r)) return 1;
    lsq_report(h, r, n_src, pose, converged);
    h->stats.attempts = r.passes;
    arm_fitness(h, pose, n_src, stride_floats);
    return 0;
}

// ---- gicp's row of the method table (handle.h: MethodOps) ----
int gicp_scan2map(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged) {
    // the whole target, every call: its index and covariances queued first, the scan's side while the host waits for the headers (as vgicp_scan2map)
    bool src_queued = false;
    const std::function<int()> queue_src = [&]() -> int { src_queued = true; return vgicp_source_enqueue(h, d_src, n_src, stride_floats, true); };
    int prc = vgicp_source_mark(h);
    if (!prc) prc = gicp_prepare_target(h, d_dst, n_dst, stride_floats, &queue_src);
    if (!prc && !src_queued) prc = queue_src();
    if (prc) { (void)side_drain(h); return 1; }
    if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_index, h->stream));
    if (run_gicp(h, d_src, n_src, stride_floats, pose, converged)) { (void)side_drain(h); return 1; }
    return end_timed_call(h);
}
int gicp_kept_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) { return gicp_prepare_target(h, d_dst, n_dst, stride_floats); }      // (never sharded: nothing to agree on)
int gicp_align(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) { return align_beside_scan_side(h, d_src, n_src, stride_floats, pose, converged, run_gicp); }
// the resolution is the cell of its index, k_corr the neighbourhood of its covariances, the regularisation shaped them; the gate and the optimiser
// settings are read at every call
bool gicp_target_from_changed(const pcr_params& old_p, const pcr_params& new_p) { return new_p.vgicp_resolution != old_p.vgicp_resolution || new_p.vgicp_k_corr != old_p.vgicp_k_corr || new_p.vgicp_regularization != old_p.vgicp_regularization; }

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_gicp_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double pose[16], const double* pose_eval,
                       double H[36], double b[6], double* error, double* error_eval, int64_t* n_corr, int32_t* corr, float* d2, double* mahal6) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kGicp) return fail(h, "pcr_gicp_linearize needs a gicp handle");
    if (!pose || !H || !b) return fail(h, "pose, H or b is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->target_ready || !h->have_target) return fail(h, "no target: call pcr_set_target first");
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    if (gicp_setup(h, d_src, n_src, stride_bytes / 4)) { (void)side_drain(h); return 1; }
    H_TRY(h->gi.d2.reserve((n_src + 1) * sizeof(float)));
    GicpArgs a = gicp_args(h, d_src, n_src, stride_bytes / 4);
    a.d2_out = h->gi.d2.as<float>();
    Pose16 T;
    memcpy(T.m, pose, sizeof T.m);
    H_TRY(gicp_launch_linearize(a, T, h->out32.dev, h->stream));
    std::vector<uint32_t> cr(n_src);
    if (n_src) {
        H_TRY(hipMemcpyAsync(cr.data(), a.corr, n_src * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        if (d2) H_TRY(hipMemcpyAsync(d2, a.d2_out, n_src * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (mahal6) H_TRY(hipMemcpyAsync(mahal6, a.corr_M, n_src * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    H_TRY(hipStreamSynchronize(h->stream));
    unpack_lsq_sums(h->out32.host, H, b, error);
    int64_t nc = 0;
    for (size_t i = 0; i < n_src; ++i) {
        const bool has = cr[i] != 0xffffffffu;
        nc += has;
        if (corr) corr[i] = has ? (int32_t)cr[i] : -1;
        // (the matrix of a point without a correspondence is whatever the buffer held: reported as zeros)
        if (mahal6 && !has) for (int k = 0; k < 6; ++k) mahal6[i * 6 + k] = 0.0;
    }
    if (n_corr) *n_corr = nc;
    if (pose_eval) {      // compute_error(pose_eval) on the correspondences just made (the trial pass; its own linearisation goes to the other buffer)
        Pose16 Te;
        memcpy(Te.m, pose_eval, sizeof Te.m);
        a.d2_out = nullptr;
        H_TRY(gicp_launch_error(a, Te, h->out32.dev, h->stream));
        H_TRY(hipStreamSynchronize(h->stream));
        if (error_eval) *error_eval = h->out32.host[28];
    } else if (error_eval) *error_eval = 0.0;
    return 0;
}

}  // extern "C"
