// lsq_host.h -- what the host drivers of the methods on fast_gicp::LsqRegistration's loop share (vgicp_host.hip, gicp_host.hip): the
// Levenberg-Marquardt driver over the state machine of vgicp_opt.h, on the device or on the host, the search cell of a map-sized target's
// covariances, the layout of a pass's sums (liorf_host.hip takes that and the pace of the device loop from here).  The device side is lsq_pass.h.
#pragma once
#include <algorithm>

#include "handle.h"

namespace pcr {
namespace host {

struct LsqResult {
    Pose16 x0;               // final_transformation_: through a Matrix4f
    bool conv = false, on_device = false;
    int outer = 0, n_lin = 0, n_err = 0, passes = 0;
    int roi_escapes = 0;     // device loop only (VgOut::roi_escapes)
};

// PCL's align() around LsqRegistration::computeTransformation from the guess `pose`.
// on_device: the device-resident loop -- launches are enqueued ahead of the device by `rule`, the host watches a progress word;
//   device_pass(i, d_ctl2, d_out, seq) queues launch i.  d_roi_escapes: a counter that starts at zero with the state, or nullptr.
// else the host-driven loop: the same state machine, one host round trip per pass; host_pass(kind, parity, xi, seq) queues a pass at xi and
//   the fold of its rows into h->out32 (parity: the two correspondence buffers have changed places); over_ranks: a sharded target, whose sums
//   cross the ranks after every pass.
template <class DevicePass, class HostPass>
int run_lsq(pcr_handle* h, const double pose[16], bool on_device, const PaceRule& rule, const char* budget_msg, DevicePass&& device_pass,
            HostPass&& host_pass, LsqResult* r, bool over_ranks = false, uint32_t* d_roi_escapes = nullptr) {
    const pcr_params& p = h->prm;
    Pose16 x0;
    for (int i = 0; i < 16; ++i) x0.m[i] = (double)(float)pose[i];     // guess handed over as Matrix4f (VgicpRegister.cpp:36)
    r->on_device = on_device;
    if (on_device) {
        H_TRY(h->lsq_out.ensure());
        H_TRY(h->lsq_ctl.reserve(2 * sizeof(VgCtl)));
        VgCtl* d_ctl = h->lsq_ctl.as<VgCtl>();
        const VgOut* out = h->lsq_out.host;
        h->seq += 1.0;
        const double seq = h->seq;
        H_TRY(vgicp_launch_ctl_init(d_ctl, x0, p.vgicp_max_iters, p.vgicp_lm_inner, p.vgicp_lm_init_scale, p.vgicp_rot_eps, p.vgicp_trans_eps, h->stream, d_roi_escapes));
        // every outer iteration takes at most lm_inner passes, plus the first linearisation and the launch that finishes
        const long limit = (long)p.vgicp_max_iters * std::max(1, p.vgicp_lm_inner) + 3;
        if (pace_passes(h, out, seq, limit, rule, "vgicp_max_iters * vgicp_lm_inner exceeds the device loop's pass window (2^20)", budget_msg,
                        [&](long i) -> hipError_t { return device_pass(i, d_ctl, h->lsq_out.dev, seq); }))
            return 1;
        x0 = out->x0; r->conv = out->conv != 0;
        r->outer = out->outer; r->n_lin = out->n_lin; r->n_err = out->n_err; r->passes = out->passes; r->roi_escapes = out->roi_escapes;
    } else {
        VgCtl c;
        memset(&c, 0, sizeof c);
        vg_opt::ctl_init(&c, x0, p.vgicp_max_iters, p.vgicp_lm_inner, p.vgicp_lm_init_scale, p.vgicp_rot_eps, p.vgicp_trans_eps);
        while (!c.done) {
            h->seq += 1.0;
            H_TRY(host_pass(c.kind, c.parity, c.xi, h->seq));
            if (wait_result(h, &h->out32.host[31], h->seq)) return 1;
            if (over_ranks && ranks_allreduce(h, h->out32.host, 29)) return 1;
            double sums[29];
            for (int k = 0; k < 29; ++k) sums[k] = h->out32.host[k];
            vg_opt::ctl_step(&c, sums);
        }
        x0 = c.x0; r->conv = c.conv != 0;
        r->outer = c.outer; r->n_lin = c.n_lin; r->n_err = c.n_err; r->passes = c.passes;
    }
    for (int i = 0; i < 16; ++i) r->x0.m[i] = (double)(float)x0.m[i];     // final_transformation_ is a Matrix4f
    return 0;
}
// the device loop of an unsharded target: a pass is ~14 us, and the word that says one has begun is written ~6 us into it: with fewer than
// three launches ahead of that word the queue runs dry while the host enqueues; a launch beyond the end costs ~5 us
static constexpr PaceRule kLsqPace{4, 3, 4, false};

// The call's result and stats.  pcr_stats.attempts stays with the callers, who differ: both report the passes the device loop evaluated,
// and after the host-driven loop GICP reports its passes there too while VGICP leaves the 0 the stats were cleared to.
inline void lsq_report(pcr_handle* h, const LsqResult& r, size_t n_src, double pose[16], int* converged) {
    memcpy(pose, r.x0.m, sizeof r.x0.m);
    if (converged) *converged = r.conv ? 1 : 0;
    h->stats.iterations = r.outer; h->stats.n_src = (int64_t)n_src; h->stats.n_dst = (int64_t)h->tgt_n;
    h->stats.kernel_launches = r.n_lin + r.n_err;
}

// A map-sized cloud's covariances are searched on ONE level whose cell is sized for the 20-neighbour radius, not for the voxel lattice:
// sum_sq / n is the occupancy of the cell a point lives in (averaged over the points); on a surface it grows with cell^2, and ~10
// points per cell put ~4 K candidates into the 27-cell block (measured optimum).  (0.5 m voxels over a 0.5 m-spaced map: cell 1.25 m,
// 0.74 -> 0.50 ms for 1 M points, the extra index build included.)  hdr0: the header of the lattice's build, with its density figure.
// Returns the cell of that level in lattice cells, or 0 when the lattice itself serves.
inline double cov_search_scale(const GridHeader& hdr0, size_t n) {
    if (cov_levels(n) != 1 || n == 0 || !(grid_sum_sq(hdr0) > 0.0)) return 0.0;
    const double occ = grid_sum_sq(hdr0) / (double)n;
    const double scale = std::min(8.0, sqrt(10.0 / std::max(occ, 1e-3)));
    return scale >= 1.3 ? scale : 0.0;
}

// the sums of a linearisation as a pass leaves them: H's upper triangle [0..20], b [21..26], the error [27]
inline void unpack_lsq_sums(const double* out32, double H[36], double b[6], double* error) {
    int q = 0;
    for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { H[r * 6 + c] = H[c * 6 + r] = out32[q++]; }
    for (int r = 0; r < 6; ++r) b[r] = out32[21 + r];
    if (error) *error = out32[27];
}

}  // namespace host
}  // namespace pcr
