// capi.hip -- the C ABI of libpcr_hip.so (include/pcr_hip.h): handle management, the method table, what the scan2map / set_target /
// align entry points do for every method before they go through it, the getters and setters.  What a method does behind its row of the
// table is in its own *_host.hip unit, as are the other entry points (handle.h lists the units); no entry point here picks a driver or a readiness flag by naming a method.
// Host C++ only talks to the kernels through the launchers in pcr_internal.h.

#include <string.h>

#include "handle.h"

using namespace pcr;
using namespace pcr::host;

namespace pcr {
namespace host {

thread_local std::string g_create_error;

// One row per Method, in the enum's order.  pcr_fitness of liorf is liorf_scan2map.cpp's own score (:22-54): d2 <= 1.0f counted, -1 when none is.
static const MethodOps kMethods[] = {
    {"loam", true, false, false, DBL_MAX, DBL_MAX, loam_scan2map, loam_prepare_target, loam_align, loam_target_from_changed},
    {"ndt", true, true, false, DBL_MAX, DBL_MAX, ndt_scan2map, ndt_kept_target, run_ndt, ndt_target_from_changed},
    {"vgicp", true, true, true, DBL_MAX, DBL_MAX, vgicp_scan2map, vgicp_kept_target, vgicp_align, vgicp_target_from_changed},
    {"gicp", false, true, true, DBL_MAX, DBL_MAX, gicp_scan2map, gicp_kept_target, gicp_align, gicp_target_from_changed},
    {"liorf", false, true, true, 1.0, -1.0, liorf_scan2map, liorf_prepare_target, run_liorf, liorf_target_from_changed},
};
const MethodOps& ops(const pcr_handle* h) { return kMethods[h->method]; }

// the call's times from the events recorded at its start, after its target index and at its end (profiling level >= 1)
int read_call_times(pcr_handle* h) {
    float ms = 0;
    H_TRY(hipEventElapsedTime(&ms, h->ev_start, h->ev_end)); h->stats.total_ms = ms;
    H_TRY(hipEventElapsedTime(&ms, h->ev_start, h->ev_index)); h->stats.index_ms = ms;
    H_TRY(hipEventElapsedTime(&ms, h->ev_index, h->ev_end)); h->stats.solve_ms = ms;
    return 0;
}

// profiling passes: the counters cleared (on the handle's stream, ahead of everything the call queues), the covariance events made
static int prof_begin(pcr_handle* h) {
    h->ev_cov_tgt_used = h->ev_cov_src_used = false; h->nd_prof_launches = 0;
    h->stats.aux_kernel_ms = 0; h->stats.region_points = h->stats.region_voxels = h->stats.pairs_grad = h->stats.pairs_hess = 0;
    if (h->profile < 2) return 0;
    H_TRY(h->prof_count.reserve(64 * sizeof(uint32_t)));
    H_TRY(hipMemsetAsync(h->prof_count.p, 0, 64 * sizeof(uint32_t), h->stream));
    for (hipEvent_t& e : h->ev_cov) if (!e) H_TRY(hipEventCreate(&e));
    return 0;
}
// ... read back once the call's work has drained
static int prof_end(pcr_handle* h) {
    if (h->profile < 2 || !h->prof_count.p) return 0;
    uint32_t c[64];
    H_TRY(hipStreamSynchronize(h->stream));
    if (h->side_stream) H_TRY(hipStreamSynchronize(h->side_stream));
    H_TRY(hipMemcpy(c, h->prof_count.p, sizeof c, hipMemcpyDeviceToHost));
    h->stats.region_points = c[0]; h->stats.region_voxels = c[16]; h->stats.pairs_grad = c[32]; h->stats.pairs_hess = c[48];
    float ms = 0;
    if (h->ev_cov_tgt_used) { H_TRY(hipEventElapsedTime(&ms, h->ev_cov[0], h->ev_cov[1])); h->stats.kernel_ms = ms; h->stats.kernel_launches = 1; }
    if (h->ev_cov_src_used) {
        h->stats.aux_kernel_ms = 0;
        for (int k = 0; k < 3; ++k) { H_TRY(hipEventElapsedTime(&ms, h->ev_cov[2 + 2 * k], h->ev_cov[3 + 2 * k])); h->stats.aux_kernel_ms += ms; }
    }
    if (h->nd_prof_launches > 0) {
        h->stats.kernel_ms = 0;
        for (int k = 0; k < h->nd_prof_launches; ++k) { H_TRY(hipEventElapsedTime(&ms, h->ev_kernel[2 * k], h->ev_kernel[2 * k + 1])); h->stats.kernel_ms += ms; }
        h->stats.kernel_launches = h->nd_prof_launches;
    }
    return 0;
}

// ... the end of a timed scan2map call (the methods whose passes are profiled): its end recorded and waited for, its times and counters read
int end_timed_call(pcr_handle* h) {
    if (h->profile < 1) return 0;
    H_TRY(hipEventRecord(h->ev_end, h->stream));
    H_TRY(hipEventSynchronize(h->ev_end));
    if (read_call_times(h)) return 1;
    return prof_end(h);
}

}  // namespace host
}  // namespace pcr

namespace {

int do_scan2map(pcr_handle* h, const void* src, size_t n_src, const void* dst, size_t n_dst, size_t stride_bytes,
                double pose[16], int* converged, bool on_device) {
    if (!h) return 1;
    h->err.clear();
    drop_fitness_state(h);
    h->map_id = 0; h->map_gen = 0;      // whatever target structures exist after this call were not built from a pcr_map generation
    if (!pose) return fail(h, "pose_inout is NULL");
    if ((n_src && !src) || (n_dst && !dst)) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    drop_query_index(h);      // (from here on the target is replaced: the staging area is written over next)
    const float *d_src, *d_dst;
    if (ops(h).passes_profiled && prof_begin(h)) return 1;
    if (h->profile >= 1) H_TRY(hipEventRecord(h->ev_start, h->stream));
    if (on_device) { d_src = (const float*)src; d_dst = (const float*)dst; }
    else {
        if (stage_host(h, &h->tgt_stage, dst, n_dst, stride_bytes, &d_dst)) return 1;
        if (stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    }
    return ops(h).scan2map(h, d_src, n_src, d_dst, n_dst, stride_bytes / 4, pose, converged);
}

// target structures of the handle's method from points in HBM that outlive them (the staging copy of pcr_set_target, or a
// pcr_map's sub-map for as long as its generation lasts)
int prepare_target_from(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_bytes) {
    h->map_id = 0; h->map_gen = 0;      // (pcr_scan2map_submap sets them after a successful preparation)
    drop_query_index(h);
    return ops(h).prepare_target(h, d_dst, n_dst, stride_bytes / 4);
}

}  // namespace

namespace pcr {
namespace host {

// The reference keeps its target after scan2Map (setInputTarget holds the cloud; test/align.cpp aligns and scores against it afterwards).  A
// pcr_scan2map of an NDT / VGICP handle prepares the target for that scan's region only (RoiView): a later pcr_align, pcr_vgicp_linearize or
// pcr_ndt_derivatives on the same target finds it prepared IN FULL here -- from this handle's own staging copy when the target came in as a host
// buffer (the plugin adapter's path).  A device buffer is the caller's and may be gone: that case asks for pcr_set_target / full_target.
int ensure_full_target(pcr_handle* h) {
    if (!h->roi_on) return 0;
    if (h->tgt_ptr != h->tgt_stage.as<float>() || !h->tgt_n || sharded(h))
        return fail(h, "no target: pcr_scan2map prepared this device-resident target for that one scan only; call pcr_set_target (or set pcr_params.full_target) "
                       "for a target that is kept");
    const uint64_t id = h->map_id, gen = h->map_gen;
    if (prepare_target_from(h, h->tgt_stage.as<float>(), h->tgt_n, h->tgt_stride * sizeof(float))) return 1;
    h->map_id = id; h->map_gen = gen;
    return 0;
}

}  // namespace host
}  // namespace pcr

namespace {
// fast_gicp's two settings (gicp_settings.hpp:6,10): the field that is out of range, named; nullptr when both are in range
const char* settings_out_of_range(const pcr_params& p) {
    if (p.vgicp_regularization < PCR_REG_NONE || p.vgicp_regularization > PCR_REG_FROBENIUS)
        return "vgicp_regularization must be 0 (NONE), 1 (MIN_EIG), 2 (NORMALIZED_MIN_EIG), 3 (PLANE) or 4 (FROBENIUS)";
    if (p.vgicp_voxel_mode < PCR_VOXEL_ADDITIVE || p.vgicp_voxel_mode > PCR_VOXEL_MULTIPLICATIVE)
        return "vgicp_voxel_mode must be 0 (ADDITIVE), 1 (ADDITIVE_WEIGHTED) or 2 (MULTIPLICATIVE)";
    // pclomp::NeighborSearchMethod (ndt_omp.h:52-57).  Every handle is checked, as with the two above; only ndt handles read the value.
    if (p.ndt_search < PCR_NDT_KDTREE || p.ndt_search > PCR_NDT_DIRECT1)
        return "ndt_search must be 1 (DIRECT26), 2 (DIRECT7) or 3 (DIRECT1); 0 (KDTREE) is not served";
    if (p.ndt_search == PCR_NDT_KDTREE)
        return "ndt_search = 0 (KDTREE) is not served: the reference searches a kd-tree over float centroids summed in input order (the result "
               "depends on the order of the target's rows), returns voxels its own covariance test rejected, and needs FLANN; use 1 (DIRECT26), "
               "2 (DIRECT7) or 3 (DIRECT1)";
    // fast_gicp::NeighborSearchMethod (gicp_settings.hpp:8).  Every handle is checked; only vgicp handles read the value.
    if (p.vgicp_search < PCR_VGICP_DIRECT27 || p.vgicp_search > PCR_VGICP_DIRECT_RADIUS)
        return "vgicp_search must be 0 (DIRECT27), 1 (DIRECT7) or 2 (DIRECT1); 3 (DIRECT_RADIUS) is not served";
    if (p.vgicp_search == PCR_VGICP_DIRECT_RADIUS)
        return "vgicp_search = 3 (DIRECT_RADIUS) is not served: the reference implements it in its CUDA variant only (gicp_settings.hpp:8) and "
               "FastVGICP aborts on it (fast_vgicp_voxel.hpp:13-15); use 0 (DIRECT27), 1 (DIRECT7) or 2 (DIRECT1)";
    if (p.query_index != PCR_QUERY_INDEX_AUTO && p.query_index != PCR_QUERY_INDEX_SPARSE) return "query_index must be 0 (AUTO) or 1 (SPARSE)";
    // liorf_scan2map.cpp's constants.  Every handle is checked; only liorf handles read the values.
    return liorf_params_out_of_range(p);
}
}  // namespace

extern "C" {

void pcr_default_params(pcr_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(pcr_params);
    p->device = -1;
    p->loam_iters = 8; p->loam_early_exit = 1;
    p->loam_knn_max_sq = (double)1.0f; p->loam_plane_thresh = (double)0.2f; p->loam_point_thresh = (double)0.1f;
    p->loam_pos_conv = (double)5e-3f; p->loam_rot_conv = (double)5e-3f;
    p->ndt_resolution = 1.0; p->ndt_step_size = 0.1; p->ndt_outlier_ratio = 0.55; p->ndt_trans_eps = 0.1;
    p->ndt_max_iters = 35; p->ndt_min_points = 6;
    p->vgicp_resolution = 1.0; p->vgicp_k_corr = 20; p->vgicp_max_iters = 64; p->vgicp_lm_inner = 10;
    p->vgicp_rot_eps = 2e-3; p->vgicp_trans_eps = 5e-4; p->vgicp_lm_init_scale = 1e-9;
    p->record_trace = 0;
    p->gicp_max_corr_dist = (double)FLT_MAX;
    p->vgicp_regularization = PCR_REG_PLANE; p->vgicp_voxel_mode = PCR_VOXEL_ADDITIVE;
    p->ndt_search = PCR_NDT_DIRECT7;
    p->vgicp_search = PCR_VGICP_DIRECT1;
    // liorf_scan2map.cpp: :392, :186, :207, :224, :268, :388, :379, :342 (the thresholds are its double literals)
    p->liorf_iters = 30; p->liorf_knn_max_sq = 1.0; p->liorf_plane_thresh = 0.2; p->liorf_point_thresh = 0.1;
    p->liorf_min_rows = 50; p->liorf_min_scan = 30; p->liorf_rot_conv_deg = 0.05; p->liorf_trans_conv_cm = 0.05;
    p->liorf_degenerate_eig = 100.0;
}

pcr_handle* pcr_create(const char* method, const pcr_params* p) {
    g_create_error.clear();
    if (!method) { g_create_error = "method is NULL"; return nullptr; }
    int m = 0;
    while (m <= kLiorf && strcmp(method, kMethods[m].name)) ++m;
    if (m > kLiorf) {
        // the reference factory throws on an unknown frontend.pcr (LidarOdometry.cpp:50-54)
        g_create_error = std::string("such pcr type(") + method + ") is not exist";
        return nullptr;
    }
    pcr_handle* h = new pcr_handle();
    h->method = (Method)m;
    pcr_default_params(&h->prm);
    if (p) {
        if (p->struct_size != sizeof(pcr_params)) { g_create_error = "pcr_params.struct_size mismatch (call pcr_default_params first)"; delete h; return nullptr; }
        h->prm = *p;
    }
    // (before any device is touched: a machine without a GPU reports the bad field, not the missing device)
    if (const char* bad = settings_out_of_range(h->prm)) { g_create_error = bad; delete h; return nullptr; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        delete h; return nullptr;
    }
    if (h->prm.device >= 0) h->device = h->prm.device;
    else if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
    if (h->device >= ndev) { g_create_error = "device ordinal out of range"; delete h; return nullptr; }
    if ((e = hipSetDevice(h->device)) != hipSuccess || (e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&h->ev_start)) != hipSuccess || (e = hipEventCreate(&h->ev_index)) != hipSuccess ||
        (e = hipEventCreate(&h->ev_end)) != hipSuccess) {
        g_create_error = std::string("HIP initialisation failed: ") + hipGetErrorString(e);
        delete h; return nullptr;
    }
    h->own_stream = true;
    memset(&h->stats, 0, sizeof(h->stats));
    return h;
}

void pcr_destroy(pcr_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    // nothing may still run when the memory goes: the device buffers and host-mapped blocks free themselves with the handle
    for (hipStream_t s : {h->stream, h->side_stream, h->vg.aux_stream}) if (s) (void)hipStreamSynchronize(s);
    if (h->stream) pin_forget_stream(h->stream);
    comm_release(h);
    if (h->vf.ret) (void)hipHostFree(h->vf.ret);
    if (h->side_hdr) (void)hipHostFree(h->side_hdr);
    for (hipEvent_t e : h->ev_kernel) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_cov) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->ev_start, h->ev_index, h->ev_end, h->ev_side_in, h->ev_side_done, h->vg.ev_hdr, h->vg.ev_aux_in, h->vg.ev_aux_done}) if (e) (void)hipEventDestroy(e);
    if (h->vg.aux_stream) (void)hipStreamDestroy(h->vg.aux_stream);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* pcr_last_error(const pcr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pcr_scan2map(pcr_handle* h, const void* src, size_t n_src, const void* dst, size_t n_dst, size_t stride_bytes,
                 double pose_inout[16], int* converged) {
    return do_scan2map(h, src, n_src, dst, n_dst, stride_bytes, pose_inout, converged, false);
}

int pcr_scan2map_device(pcr_handle* h, const void* d_src, size_t n_src, const void* d_dst, size_t n_dst,
                        size_t stride_bytes, double pose_inout[16], int* converged) {
    return do_scan2map(h, d_src, n_src, d_dst, n_dst, stride_bytes, pose_inout, converged, true);
}

int pcr_set_target(pcr_handle* h, const void* dst, size_t n_dst, size_t stride_bytes, int on_device) {
    if (!h) return 1;
    h->err.clear();
    if (n_dst && !dst) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    drop_query_index(h);      // (before the staging copy it was built from is written over: a copy that fails must not leave it standing)
    // the library copies what it keeps: the index holds its own sorted copy, but a rebuild after a
    // cell-table overflow needs the raw points, so they are staged in HBM either way
    const size_t bytes = n_dst * stride_bytes;
    if (on_device) {
        H_TRY(h->tgt_stage.reserve(bytes ? bytes : 16));
        if (bytes) H_TRY(hipMemcpyAsync(h->tgt_stage.p, dst, bytes, hipMemcpyDeviceToDevice, h->stream));
    } else {
        const float* staged = nullptr;
        if (stage_host(h, &h->tgt_stage, dst, n_dst, stride_bytes, &staged)) return 1;
    }
    return prepare_target_from(h, h->tgt_stage.as<float>(), n_dst, stride_bytes);
}

int pcr_scan2map_submap(pcr_handle* h, const void* src, size_t n_src, int src_on_device, const pcr_map* m, double pose_inout[16],
                        int* converged) {
    if (!h) return 1;
    h->err.clear();
    if (!m) return fail(h, "map is NULL");
    uint64_t id = 0, gen = 0;
    size_t n_dst = 0, stride_bytes = 0;
    if (pcr_map_generation(m, &id, &gen)) return fail(h, "map is not usable");
    const void* d_dst = pcr_map_submap(m, &n_dst, &stride_bytes);
    if (!d_dst || n_dst == 0 || stride_bytes == 0) {
        // an empty sub-map (no key frame selected yet): the ordinary entry point defines what registration against nothing returns
        if (stride_bytes == 0) stride_bytes = 16;
        pcr_invalidate_target(h);
        return do_scan2map(h, src, n_src, nullptr, 0, stride_bytes, pose_inout, converged, src_on_device != 0);
    }
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    const bool current = h->map_id == id && h->map_gen == gen && h->have_target && target_prepared(h);
    // Sharded: prepare_target_from() ends in a collective (agree_prepared), so either every rank rebuilds or none does -- a rank
    // whose tile index was cut, or whose map is at another generation, must not enter that exchange while its peers are already
    // summing normal equations.  One MAX over the ranks of "I have to rebuild" decides for all.
    double need = current ? 0.0 : 1.0;
    if (sharded(h) && ranks_allreduce(h, &need, 1, 1)) return 1;
    if (need != 0.0) {
        // VGICP, a scan that is in HBM already: its side goes onto the side stream FIRST and runs beside the new sub-map's preparation (clouds of a few ten
        // thousand points: the device is mostly idle behind either)
        if (vgicp_family(h) && !sharded(h) && src_on_device && n_src > 0 && src && vgicp_source_enqueue(h, static_cast<const float*>(src), n_src, stride_bytes / 4)) return 1;
        if (prepare_target_from(h, static_cast<const float*>(d_dst), n_dst, stride_bytes)) {
            (void)side_drain(h);      // (nothing of this call stays in flight)
            return 1;
        }
        h->map_id = id; h->map_gen = gen;
        h->target_builds += 1;
    }
    return pcr_align(h, src, n_src, stride_bytes, src_on_device, pose_inout, converged);
}

int pcr_align(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, double pose_inout[16],
              int* converged) {
    if (!h) return 1;
    h->err.clear();
    if (!pose_inout) return fail(h, "pose_inout is NULL");
    if (n_src && !src) return fail(h, "NULL cloud with nonzero size");
    if (check_stride(h, stride_bytes) || set_device(h)) return 1;
    if (!h->have_target || !h->grid.valid) return fail(h, "no target: call pcr_set_target first");
    if (ensure_full_target(h)) return 1;
    drop_fitness_state(h);
    const float* d_src = (const float*)src;
    if (!on_device && stage_host(h, &h->src_stage, src, n_src, stride_bytes, &d_src)) return 1;
    return ops(h).align(h, d_src, n_src, stride_bytes / 4, pose_inout, converged);
}

int pcr_invalidate_target(pcr_handle* h) {
    if (!h) return 1;
    h->have_target = false; h->grid.valid = false; h->target_ready = false;
    h->map_id = 0; h->map_gen = 0; h->roi_on = false;
    drop_query_index(h);
    return 0;
}

int pcr_get_stats(pcr_handle* h, pcr_stats* out) {
    if (!h || !out) return 1;
    *out = h->stats;
    out->target_builds = (int32_t)h->target_builds;
    out->region_repeats = (int32_t)h->roi_repeats; out->region_index = (h->roi_on && h->grid.filtered) ? 1 : 0;
    out->index_box_hint = h->grid.used_hint ? 1 : 0; out->index_layout_hint = h->grid.used_layout ? 1 : 0;
    return 0;
}

int pcr_set_profile(pcr_handle* h, int level) {
    if (!h) return 1;
    h->profile = level < 0 ? 0 : (level > 2 ? 2 : level);
    return 0;
}

int pcr_set_stream(pcr_handle* h, void* hip_stream) {
    if (!h) return 1;
    if (h->stream) { (void)hipStreamSynchronize(h->stream); pin_forget_stream(h->stream); }      // (copies out of pinned ranges are noted per stream)
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    return 0;
}

int pcr_get_params(const pcr_handle* h, pcr_params* out) {
    if (!h || !out) return 1;
    *out = h->prm;
    return 0;
}

int pcr_set_params(pcr_handle* h, const pcr_params* p) {
    if (!h) return 1;
    h->err.clear();
    if (!p) return fail(h, "params is NULL");
    if (p->struct_size != sizeof(pcr_params)) return fail(h, "pcr_params.struct_size mismatch (start from pcr_get_params or pcr_default_params)");
    if (p->device >= 0 && p->device != h->device) return fail(h, "a handle cannot move to another device");
    if (vgicp_family(h) && p->vgicp_k_corr != 20) return fail(h, "this build supports vgicp_k_corr = 20 (the reference's value) only");
    if (const char* bad = settings_out_of_range(*p)) return fail(h, bad);
    // ndt_search: the voxel Gaussians do not depend on the neighbourhood, so the prepared target stays; the halo of a sharded handle was
    // checked against the old setting and is checked again (nothing has been changed yet when it does not hold)
    if (h->method == kNdt && h->use_tile && h->have_halo && p->ndt_search != h->prm.ndt_search) {
        const double need = ndt_halo_need(p->ndt_search, (double)(float)p->ndt_resolution);
        if (h->halo < need * (1.0 - 1e-12)) return fail(h, ndt_halo_message(p->ndt_search, need));
    }
    // vgicp_search: the voxels do not depend on the neighbourhood, so the prepared target stays (the next call sizes the correspondence buffers by
    // the setting in force); a sharded handle serves DIRECT1 only (nothing has been changed yet when it is refused)
    if (const char* no = vgicp_search_shard_refusal(h, p->vgicp_search, false)) return fail(h, no);
    const pcr_params old = h->prm;
    h->prm = *p;
    h->prm.device = old.device;
    // whatever was derived from a parameter that changed is dropped (each method's unit says what its target is derived from); the optimiser
    // settings are read at every call.  (A loam handle never sets target_ready: there is none to clear.)
    if (ops(h).target_from_changed(old, *p)) { h->target_ready = false; h->have_target = false; h->grid.valid = false; drop_query_index(h); }
    // the regularisation shaped every covariance the handle holds: a scan's side that is still in flight (pcr_scan2map_submap queues it ahead) is
    // collected and forgotten -- its covariances are the old setting's
    const bool reg_changed = p->vgicp_regularization != old.vgicp_regularization;
    if (reg_changed && vgicp_family(h) && h->side_pending && !set_device(h)) (void)side_drain(h);
    return 0;
}

}  // extern "C"

hipStream_t pcr_internal_stream(const pcr_handle* h) { return h ? h->stream : nullptr; }

