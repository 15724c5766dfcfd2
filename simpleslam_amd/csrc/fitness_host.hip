// fitness_host.hip -- getFitnessScore() as a call of its own: the scan and the pose an alignment keeps for it (the drivers of the methods whose
// row of the method table says scores_kept_scan) and pcr_fitness, which evaluates the score when asked.

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

// a new registration starts: whatever pcr_fitness() could evaluate belongs to the previous one (a call that fails during
// target preparation must not leave the new scan's points paired with the old pose)
void drop_fitness_state(pcr_handle* h) { h->fit_pending = false; h->fit_n = 0; h->fit_copied_from = nullptr; h->fitness = -1.0; }

// An alignment of scan d_src begins: whatever score was pending is dropped.  Returns whether fit_src holds this very scan already (the side
// stream copied it: vgicp_source_enqueue).
bool fitness_scan_kept(pcr_handle* h, const float* d_src) {
    h->fit_pending = false;
    const bool kept = h->fit_copied_from == d_src && d_src != nullptr;
    h->fit_copied_from = nullptr;
    return kept;
}
// ... and once the scan's side has settled, an unsharded handle keeps the scan for a later pcr_fitness()
int keep_scan_for_fitness(pcr_handle* h, const float* d_src, size_t n, size_t stride_floats, bool kept) {
    if (kept || sharded(h) || n == 0) return 0;
    H_TRY(h->fit_src.reserve(n * stride_floats * sizeof(float)));
    H_TRY(hipMemcpyAsync(h->fit_src.p, d_src, n * stride_floats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
// pcl::Registration::getFitnessScore() of that scan at `pose` is evaluated when asked for (pcr_fitness), as in the reference
void arm_fitness(pcr_handle* h, const double pose[16], size_t n, size_t stride_floats) {
    for (int i = 0; i < 16; ++i) h->fit_pose[i] = pose[i];
    h->fit_n = n; h->fit_stride = stride_floats; h->fit_pending = true;
    h->fitness = DBL_MAX;
}

}  // namespace host
}  // namespace pcr

extern "C" double pcr_fitness(pcr_handle* h) {
    if (!h) return -1.0;
    // PointCloudRegister::getFitnessScore() returns 0 unless overridden (PointCloudRegister.hpp:34);
    // only VgicpRegister overrides it (VgicpRegister.cpp:42-45); a liorf handle answers with liorf_scan2map.cpp's own getFitnessScore (:22-54)
    const MethodOps& m = ops(h);
    if (!m.scores_kept_scan) return 0.0;
    if (h->fit_pending) {
        // mean squared distance of the aligned scan to its nearest target points, against the target the handle holds NOW (PCL does
        // the same: input_ transformed by final_transformation_, searched in the current target tree)
        h->fit_pending = false;
        h->err.clear();
        h->fitness = m.fit_none;
        if (h->target_ready && h->fit_n > 0) {
            if (set_device(h) || ensure_out32(h)) return -1.0;
            // the score of the kept scan on the sparse index, which holds every point: where pcr_params.query_index asks for it, and below where
            // the dense index was cut and cannot answer (n_viol: for how many points)
            auto on_sparse = [&](double n_viol) {
                if (sparse_fitness_run(h, "pcr_fitness", n_viol, h->fit_src.as<float>(), h->fit_n, h->fit_stride, h->fit_pose, m.fit_max_sq)) {
                    h->fitness = -1.0;
                    return -1.0;
                }
                h->fitness = h->out32.host[1] > 0 ? h->out32.host[0] / h->out32.host[1] : m.fit_none;
                return h->fitness;
            };
            if (scores_on_sparse(h)) return on_sparse(0.0);
            h->seq += 1.0;
            // (a lattice that holds the scan's region only cannot answer a nearest-neighbour question; the grid its covariances were searched on holds every point)
            const bool full_search_grid = h->cov_l1.valid && !h->cov_l1.filtered;
            if (h->grid.filtered && !full_search_grid) {
                h->err = "the voxel lattice of the last pcr_scan2map holds the scan's region only (pcr_stats.region_index) and no grid of every target point is at hand";
                h->fitness = -1.0;
                return -1.0;
            }
            const GridIndex& fit_grid = h->grid.filtered ? h->cov_l1 : h->grid;
            if (fitness_launch(fit_grid, h->fit_src.as<float>(), h->fit_n, h->fit_stride, h->fit_pose, m.fit_max_sq, h->vg_partials.as<double>(),
                               h->out32.dev, h->stream, h->seq, nullptr) != hipSuccess) { h->err = "fitness_launch failed"; return -1.0; }
            if (wait_result(h, &h->out32.host[31], h->seq)) return -1.0;
            // (fitness_kernel: points whose nearest target point may lie beyond a cut face of the index)
            if (h->out32.host[2] > 0) return on_sparse(h->out32.host[2]);
            h->fitness = h->out32.host[1] > 0 ? h->out32.host[0] / h->out32.host[1] : m.fit_none;
        }
    }
    return h->fitness;
}
