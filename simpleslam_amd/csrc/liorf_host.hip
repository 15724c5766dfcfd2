// liorf_host.hip -- the liorf method's host side: LioScan2map::scan2MapOptimization of the reference's test/comp/liorf_scan2map.cpp (:385-413)
// around the launches of liorf.hip, the preparation of its target, its refusals, the two PCL functions it is defined by
// (pcr_liorf_pose_to_6dof, pcr_liorf_6dof_to_pose), pcr_liorf_linearize and pcr_liorf_result.

#include <algorithm>

#include "lsq_host.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

const char* liorf_params_out_of_range(const pcr_params& p) {
    if (p.liorf_iters < 0) return "liorf_iters must be >= 0";
    if (p.liorf_file_row != 0 && p.liorf_file_row != 1) return "liorf_file_row must be 0 (the derivative) or 1 (the file's line 310)";
    if (!(p.liorf_knn_max_sq > 0.0)) return "liorf_knn_max_sq must be > 0";
    if (!(p.liorf_plane_thresh > 0.0)) return "liorf_plane_thresh must be > 0";
    if (!std::isfinite(p.liorf_point_thresh)) return "liorf_point_thresh must be finite";
    if (p.liorf_min_rows < 0) return "liorf_min_rows must be >= 0";
    if (p.liorf_min_scan < 0) return "liorf_min_scan must be >= 0";
    if (!(p.liorf_rot_conv_deg >= 0.0)) return "liorf_rot_conv_deg must be >= 0";
    if (!(p.liorf_trans_conv_cm >= 0.0)) return "liorf_trans_conv_cm must be >= 0";
    if (!std::isfinite(p.liorf_degenerate_eig)) return "liorf_degenerate_eig must be finite";
    return nullptr;
}

// The whole target, always: an index of every finite point for the exact 5-NN.  The cell decides how many candidates a search visits,
// never a result.  A box no dense table can hold would need a cut index: refused.
int liorf_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats) {
    h->target_ready = false;
    h->have_target = false;
    h->roi_on = false;
    h->clamp.use = 0;
    if (sharded(h) || h->use_tile) return fail(h, "liorf: sharded targets are not supported in this version");
    if (n_dst > kMaxPoints) return fail(h, "liorf: target cloud too large");
    // Every linearisation reads a neighbour at its original index, so the points must live as long as the prepared target does: a device
    // buffer of the caller's is copied into the handle's own staging area first (as gicp_prepare_target does)
    if (n_dst > 0 && d_dst != h->tgt_stage.as<float>()) {
        const size_t bytes = n_dst * stride_floats * sizeof(float);
        H_TRY(h->tgt_stage.reserve(bytes));
        H_TRY(hipMemcpyAsync(h->tgt_stage.p, d_dst, bytes, hipMemcpyDeviceToDevice, h->stream));
        d_dst = h->tgt_stage.as<float>();
    }
    h->tgt_ptr = d_dst; h->tgt_n = n_dst; h->tgt_stride = stride_floats;
    h->grid.no_hints = h->prm.index_no_hints != 0;
    if (settle_grid(h, h->grid, d_dst, n_dst, stride_floats, 1.0, 0, nullptr)) {
        if (h->err.find("grid cells") != std::string::npos)
            h->err = "liorf: the target's box cannot be tabulated (" + h->err + "; a stray point far from the map?): that needs a cut index, which liorf "
                     "does not support in this version";
        else h->err = "liorf: preparing the target: " + h->err;
        return 1;
    }
    h->have_target = true;
    h->target_ready = true;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {

// The arguments of the handle's liorf launches over a source
LiorfArgs liorf_args(const pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, const float six[6]) {
    LiorfArgs a;
    memset(&a, 0, sizeof a);
    a.src = d_src; a.n_src = (uint32_t)n_src; a.src_stride = (uint32_t)stride_floats;
    a.grid = h->grid.view();
    a.tgt = h->tgt_ptr; a.tgt_stride = (uint32_t)h->tgt_stride;
    const pcr_params& p = h->prm;
    a.c.knn_max_sq = p.liorf_knn_max_sq; a.c.plane_thresh = p.liorf_plane_thresh; a.c.point_thresh = p.liorf_point_thresh;
    a.c.rot_conv_deg = p.liorf_rot_conv_deg; a.c.trans_conv_cm = p.liorf_trans_conv_cm; a.c.degenerate_eig = p.liorf_degenerate_eig;
    a.c.iters = p.liorf_iters; a.c.min_rows = p.liorf_min_rows; a.c.file_row = p.liorf_file_row;
    for (int i = 0; i < 6; ++i) a.six0[i] = six[i];
    return a;
}

// the state's and the rows' memory in place
int liorf_setup(pcr_handle* h, size_t n_src) {
    if (!h->target_ready || !h->have_target || !h->grid.valid) return fail(h, "no target prepared");
    if (sharded(h) || h->use_tile) return fail(h, "liorf: sharded handles are not supported in this version");
    if (n_src > kMaxPoints) return fail(h, "source cloud too large");
    if (ensure_out32(h)) return 1;
    H_TRY(h->lf.out.ensure());
    H_TRY(h->lf.ctl.reserve(2 * sizeof(LiorfCtl)));
    H_TRY(h->vg_partials.reserve((size_t)2 * 512 * 32 * sizeof(double)));
    return 0;
}

}  // namespace

namespace pcr {
namespace host {

int run_liorf(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged) {
    (void)fitness_scan_kept(h, d_src);
    h->lf.have_result = false;
    if (liorf_setup(h, n_src)) return 1;
    const pcr_params& p = h->prm;
    float six[6];
    (void)pcr_liorf_pose_to_6dof(pose, six);      // (:113-115) once per call, on the host
    int conv = 0, iters_run = 0, degenerate = 0, passes = 0;
    long launched = 0;
    long long rows_last = 0;
    h->loam.trace_iters = 0;
    // the scan kept for pcr_fitness(): copied ahead of the loop, so that it has been read when the loop's result arrives
    if (keep_scan_for_fitness(h, d_src, n_src, stride_floats, false)) return 1;
    const bool looped = (long long)n_src > (long long)p.liorf_min_scan && p.liorf_iters > 0;      // laserCloudSurfLastDSNum > 30 (:388)
    if (looped) {
        LiorfArgs a = liorf_args(h, d_src, n_src, stride_floats, six);
        if (p.record_trace) {
            H_TRY(h->lf.trace.reserve((size_t)p.liorf_iters * sizeof(LoamTrace)));
            H_TRY(hipMemsetAsync(h->lf.trace.p, 0, (size_t)p.liorf_iters * sizeof(LoamTrace), h->stream));
            a.trace = h->lf.trace.as<LoamTrace>();
        }
        LiorfCtl* d_ctl = h->lf.ctl.as<LiorfCtl>();
        const LiorfOut* out = h->lf.out.host;
        h->seq += 1.0;
        const double seq = h->seq;
        // launch k >= 1 consumes linearisation k - 1; the loop ends in the prologue of the launch after its last linearisation
        const long limit = (long)p.liorf_iters + 2;
        if (pace_passes(h, out, seq, limit, kLsqPace, "liorf_iters exceeds the device loop's pass window (2^20)",
                        "liorf: the optimiser did not finish within its pass budget",
                        [&](long i) -> hipError_t { ++launched; return liorf_launch_pass(a, d_ctl, h->vg_partials.as<double>(), h->lf.out.dev, h->stream, seq, (int)i); }))
            return 1;
        for (int i = 0; i < 6; ++i) six[i] = out->six[i];
        conv = out->converged; iters_run = out->iters_run; degenerate = out->degenerate; rows_last = out->rows_last; passes = out->passes;
        if (p.record_trace) {
            const int nt = std::min(iters_run, p.liorf_iters);
            h->loam.trace_host.assign((size_t)p.liorf_iters, LoamTrace{});
            H_TRY(hipStreamSynchronize(h->stream));
            if (nt > 0) H_TRY(hipMemcpy(h->loam.trace_host.data(), h->lf.trace.p, (size_t)nt * sizeof(LoamTrace), hipMemcpyDeviceToHost));
            // (a linearisation that kept too few rows solved nothing and left no record)
            h->loam.trace_iters = (rows_last < p.liorf_min_rows && nt > 0) ? nt - 1 : nt;
        }
    }
    (void)pcr_liorf_6dof_to_pose(six, pose);      // Eigen::Affine3f res = trans2Affine3f(transformTobeMapped) (:409)
    if (converged) *converged = conv;
    for (int i = 0; i < 6; ++i) h->lf.six[i] = six[i];
    h->lf.degenerate = degenerate; h->lf.rows_last = rows_last; h->lf.have_result = true;
    h->stats.iterations = iters_run; h->stats.n_src = (int64_t)n_src; h->stats.n_dst = (int64_t)h->tgt_n;
    h->stats.kernel_launches = (int32_t)launched;      // launches of liorf_iterate_kernel queued: one per linearisation, the one that ends the loop, those the pacer kept ahead
    h->stats.attempts = passes;
    if (!looped && n_src > 0) H_TRY(hipStreamSynchronize(h->stream));      // (the copy reads the caller's buffer: nothing stays in flight behind the caller's back)
    arm_fitness(h, pose, n_src, stride_floats);
    h->fitness = -1.0;
    return 0;
}

// ---- liorf's row of the method table (handle.h: MethodOps; its kept target is liorf_prepare_target -- never sharded: nothing to agree on --, its align run_liorf) ----
int liorf_scan2map(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged) {
    // kdtreeSurfFromMap->setInputCloud on every call (liorf_scan2map.cpp:390): the whole target indexed, every call
    if (liorf_prepare_target(h, d_dst, n_dst, stride_floats)) return 1;
    if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_index, h->stream));
    if (run_liorf(h, d_src, n_src, stride_floats, pose, converged)) return 1;
    return end_timed_call(h);
}
// the index has a fixed cell and holds every point: no parameter shapes it (the thresholds are read at every call)
bool liorf_target_from_changed(const pcr_params&, const pcr_params&) { return false; }

}  // namespace host
}  // namespace pcr

extern "C" {

int pcr_liorf_pose_to_6dof(const double T[16], float out6[6]) {
    if (!T || !out6) return 1;
    // the pose as a Matrix4f (column-major: entry (r, c) at c * 4 + r); pcl::getEulerAngles
    const float t00 = (float)T[0], t10 = (float)T[1], t20 = (float)T[2], t21 = (float)T[6], t22 = (float)T[10];
    out6[0] = atan2f(t21, t22);
    out6[1] = asinf(-t20);
    out6[2] = atan2f(t10, t00);
    out6[3] = (float)T[12]; out6[4] = (float)T[13]; out6[5] = (float)T[14];
    return 0;
}

int pcr_liorf_6dof_to_pose(const float in6[6], double T[16]) {
    if (!in6 || !T) return 1;
    // pcl::getTransformation(x, y, z, roll, pitch, yaw)
    const float A = cosf(in6[2]), B = sinf(in6[2]), C = cosf(in6[1]), D = sinf(in6[1]), E = cosf(in6[0]), F = sinf(in6[0]);
    float R[12];
    lf_opt::transformation(in6, A, B, C, D, E, F, R);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T[c * 4 + r] = (double)R[r * 4 + c];
    T[3] = T[7] = T[11] = 0.0; T[15] = 1.0;
    return 0;
}

int pcr_liorf_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const float six[6],
                        float T_used[16], uint8_t* kept, float* coeff4, double AtA[36], double AtB[6], int64_t* n_kept) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kLiorf) return fail(h, "pcr_liorf_linearize needs a liorf handle");
    if (!six || !AtA || !AtB) return fail(h, "six, AtA or AtB is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->target_ready || !h->have_target) return fail(h, "no target: call pcr_set_target first");
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    if (liorf_setup(h, n_src)) return 1;
    H_TRY(h->lf.kept.reserve(n_src + 16));
    H_TRY(h->lf.coeff.reserve((n_src + 1) * 4 * sizeof(float)));
    LiorfArgs a = liorf_args(h, d_src, n_src, stride_bytes / 4, six);
    a.kept_out = h->lf.kept.as<uint8_t>();
    a.coeff_out = h->lf.coeff.as<float>();
    h->seq += 1.0;
    H_TRY(liorf_launch_linearize(a, h->lf.ctl.as<LiorfCtl>(), h->vg_partials.as<double>(), nullptr, h->out32.dev, h->stream, h->seq));
    LiorfCtl c;
    H_TRY(hipMemcpyAsync(&c, h->lf.ctl.p, sizeof c, hipMemcpyDeviceToHost, h->stream));
    if (n_src) {
        if (kept) H_TRY(hipMemcpyAsync(kept, a.kept_out, n_src, hipMemcpyDeviceToHost, h->stream));
        if (coeff4) H_TRY(hipMemcpyAsync(coeff4, a.coeff_out, n_src * 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    H_TRY(hipStreamSynchronize(h->stream));
    if (wait_result(h, &h->out32.host[31], h->seq)) return 1;
    unpack_lsq_sums(h->out32.host, AtA, AtB, nullptr);
    if (n_kept) *n_kept = (int64_t)h->out32.host[27];
    if (T_used) {
        for (int i = 0; i < 12; ++i) T_used[i] = c.T[i];
        T_used[12] = T_used[13] = T_used[14] = 0.0f; T_used[15] = 1.0f;
    }
    return 0;
}

int pcr_liorf_result(pcr_handle* h, float six[6], int* degenerate, int64_t* rows_last) {
    if (!h) return 1;
    h->err.clear();
    if (h->method != kLiorf) return fail(h, "pcr_liorf_result needs a liorf handle");
    if (!h->lf.have_result) return fail(h, "liorf: no alignment yet");
    if (six) for (int i = 0; i < 6; ++i) six[i] = h->lf.six[i];
    if (degenerate) *degenerate = h->lf.degenerate;
    if (rows_last) *rows_last = (int64_t)h->lf.rows_last;
    return 0;
}

}  // extern "C"
