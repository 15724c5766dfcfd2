// handle.h -- struct pcr_handle and what the host units of the C ABI share (host code only; no kernel includes this).
// The units: capi.hip (handle, the method table, the common part of scan2map / set_target / align, getters and setters), staging_host.hip,
// comm_host.hip, one unit per method -- loam_host.hip, ndt_host.hip, vgicp_host.hip, gicp_host.hip (the two share lsq_host.h), liorf_host.hip:
// each owns the functions of its row of the table (MethodOps) --, fitness_host.hip, voxel_host.hip, voxel_sparse_host.hip, query_host.hip.
// A nested struct of the handle belongs to the unit it is named after: that unit sets it up and writes it (pcr_destroy reaches
// into all of them); where another unit looks into one, the member's comment says so.  What several units share stays at the
// top level, with its users named.
#pragma once
#include <float.h>
#include <math.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "pcr_internal.h"
#include "ndt_opt.h"
#include "vgicp_opt.h"
#include "liorf_opt.h"
#include "small_math.h"

namespace pcr {
namespace host {

enum Method { kLoam = 0, kNdt = 1, kVgicp = 2, kGicp = 3, kLiorf = 4 };

// A block of `count` T in host-mapped memory, which kernels write through `dev` and the host reads at `host`: allocated and
// zeroed on first use, freed with its owner.
template <class T> struct Mapped {
    T* host = nullptr;
    T* dev = nullptr;
    Mapped() = default;
    Mapped(const Mapped&) = delete;
    Mapped& operator=(const Mapped&) = delete;
    ~Mapped() { if (host) (void)hipHostFree(host); }
    hipError_t ensure(size_t count = 1) {
        if (host) return hipSuccess;
        hipError_t e = hipHostMalloc((void**)&host, count * sizeof(T), hipHostMallocMapped);
        if (e != hipSuccess) { host = nullptr; return e; }
        memset(host, 0, count * sizeof(T));
        if ((e = hipHostGetDevicePointer((void**)&dev, host, 0)) != hipSuccess) { (void)hipHostFree(host); host = dev = nullptr; }
        return e;
    }
};

// the most points a cloud may have (the kernels count them in 32 bits)
static constexpr size_t kMaxPoints = 0xfffffff0ull;

// LOAM ClampBox (loam_host.hip: check_grid_overflow): first room around the scan, and how often it is doubled (10 m ... 320 m)
static constexpr double kClampMargin = 10.0;
static constexpr int kClampRetries = 6;

}  // namespace host
}  // namespace pcr

struct pcr_handle {
    pcr::host::Method method = pcr::host::kLoam;
    pcr_params prm;                  // every unit
    std::string err;                 // every unit
    int device = 0;
    hipStream_t stream = nullptr;    // every unit
    bool own_stream = false;
    int profile = 1;

    // target
    pcr::GridIndex grid;             // every unit but staging, comm and voxel
    pcr::DeviceBuf tgt_stage;        // host targets are staged here (capi; query: fit_grid_for)
    const float* tgt_ptr = nullptr;   // device pointer the index was built from (for rebuild on overflow) (capi, loam, vgicp, ndt, query)
    size_t tgt_n = 0, tgt_stride = 0;
    bool have_target = false;        // capi, loam, vgicp, ndt, query
    // ndt, vgicp, gicp, liorf: the method's own target structures stand.  Set by the method's *_prepare_target alone; dropped by it, by pcr_set_params,
    // pcr_invalidate_target, pcr_set_shard (vgicp) and query's fit_grid_for (ndt).  A loam handle never sets it: read through target_prepared()
    bool target_ready = false;
    pcr::ClampBox clamp{};           // LOAM scan2map fallback: region of interest of a target whose full box cannot be tabulated (capi, loam, vgicp)
    bool clamp_allowed = false;      // set while a scan2map call (target rebuilt for this very scan) is running (capi, loam)
    bool clamp_from_bulk = false;    // pcr_set_target in progress: an untabulatable box may be cut to the bulk of the target (capi, loam)
    int clamp_bulk_stage = 0;        // ... how far that has gone: 0 not cut, 1 cut to the bulk box, 2 to the room around one point (loam)
    double clamp_margin = 10.0;      // LOAM ClampBox: room around the scan, doubled when a query reached a cut face (loam, vgicp)
    uint64_t map_id = 0, map_gen = 0;    // pcr_scan2map_submap: the sub-map the target structures were built from (capi)
    long long target_builds = 0;         // ... and how often it had to build them
    // source
    pcr::DeviceBuf src_stage;        // capi, loam, vgicp, ndt, query
    pcr::GridIndex src_grid;         // the scan's own index: VGICP's fine level (vgicp), the scan's box for a LOAM clamp (loam)

    // LOAM work memory (loam_host.hip)
    struct Loam {
        uint32_t last_blocks = 0;        // linearisation blocks of the last LOAM call (timeline readout)
        pcr::DeviceBuf state, partials, trace, reduced, dbg_status, dbg_rows, dbg_nn, nn_cache, timeline;
        pcr::host::Mapped<pcr::LoamResult> result;           // written by the finalize kernel
        std::vector<pcr::LoamTrace> trace_host;
        int trace_iters = 0;
        pcr::host::Mapped<double> red;   // kAccum doubles: the LOAM sums on their way through the caller's collective
        pcr::DeviceBuf dummy_grid;       // a GridHeader marked overflow + empty: the grid view of a rank whose index failed
    } loam;

    // the scan's side of a VGICP call, on its own stream (vgicp; capi: drained on error paths, pcr_align compares the scan queued; pcr_destroy)
    hipStream_t side_stream = nullptr;     // source index + covariances of a scan2map call, concurrent with the target preparation
    hipEvent_t ev_side_in = nullptr, ev_side_done = nullptr;
    pcr::GridHeader* side_hdr = nullptr;  // pinned: headers of the three source levels [0..2] and of the target's grids [3..6], read back without blocking the host
    bool side_pending = false;       // source work of (side_src, side_n, side_stride) is in flight on side_stream
    const float* side_src = nullptr; size_t side_n = 0, side_stride = 0;
    pcr::GridIndex cov_l1;           // the TARGET cloud while its covariances are computed, indexed at 4x the cell (vgicp; query: the grid of every point a score runs on)
    double cov_scale_hint = 0.0;     // cell scale of the last map-sized target's covariance grid: built ahead of the density it is derived from (vgicp, query)
    pcr::DeviceBuf vg_partials;      // rows of a pass's sums: vgicp, the fitness scores of vgicp and query; sized by staging (ensure_out32)
    pcr::DeviceBuf lsq_ctl;              // two VgCtl: the state of the device-resident LM loop of vgicp or gicp (lsq_host.h: run_lsq), by launch parity
    pcr::host::Mapped<pcr::VgOut> lsq_out;   // its result and progress word
    double seq = 0.0;                    // completion numbers of the host-mapped result blocks below (vgicp, ndt, query)
    pcr::host::Mapped<double> out32;     // 32 doubles written by sum_partials_kernel (staging: ensure_out32; vgicp, query)
    // getFitnessScore() is a call of its own in the reference (VgicpRegister.cpp:42-45: PCL evaluates it when asked, from the source it
    // still holds): an unsharded alignment keeps a copy of the scan and the final pose, and pcr_fitness() evaluates the score on demand
    // (fitness_host.hip; the drivers of vgicp, gicp and liorf keep the scan and arm the score; query: reloc_point_fitness_at)
    pcr::DeviceBuf fit_src;
    const float* fit_copied_from = nullptr;   // the scan fit_src holds (copied on the side stream by vgicp_source_enqueue)
    size_t fit_n = 0, fit_stride = 0;
    double fit_pose[16];
    bool fit_pending = false;
    double fitness = -1.0;

    // VGICP work memory (vgicp_host.hip)
    struct Vg {
        pcr::GridIndex cov_l2;           // the TARGET cloud while its covariances are computed, indexed at 16x the cell (4x: cov_l1)
        pcr::GridIndex src_l1, src_l2;   // the same for the source (own buffers: its side runs on side_stream next to the target's)
        hipEvent_t ev_hdr = nullptr, ev_aux_in = nullptr, ev_aux_done = nullptr;
        hipStream_t aux_stream = nullptr; // the target's covariance grid, built beside its voxel lattice (settle_cov_levels)
        pcr::GridHeader cov_hdr0;        // header of the fine level of the last settle_cov_levels (density estimate)
        bool cov_l1_ahead = false;       // ... and whether that build is the one in h->cov_l1 now
        pcr::DeviceBuf tgt_cov6, src_cov6, vox, corr_slot, corr_M, corr_slot2, corr_M2;
        pcr::DeviceBuf corr_T, corr_T2;  // pcr_params.vgicp_search = DIRECT7 / DIRECT27: the pose of the linearisation that wrote corr_slot / corr_slot2 (VgicpArgs::corr_T)
        // the last pcr_vgicp_linearize, for pcr_vgicp_correspondences: its source rows and setting (corr_slot holds its pairs); any other call over a source drops it
        bool lin_valid = false;
        size_t lin_n = 0;
        int lin_search = 0;
        pcr::CovScratch src_scratch, tgt_scratch;   // neighbour lists + queue of the covariance search of a scan-sized cloud: the source's runs on the side stream beside the target's
        pcr::DeviceBuf reduced;              // sharded VGICP over the peer exchange: a pass's 32 sums folded over the rows and the ranks
        pcr::DeviceBuf cov_viol;         // VGICP halo check: number of neighbourhoods that reach past the halo
    } vg;

    // GICP work memory (gicp_host.hip).  The scan's side -- its index levels, covariances, the copy kept for the fitness score -- is VGICP's (vg.src_*,
    // side_stream); the target is h->grid (every finite point, for the 1-NN) and h->cov_l1 / vg.cov_l2 (the levels of its covariance search).
    struct Gicp {
        pcr::DeviceBuf tgt_cov6;             // per target point, original order
        pcr::DeviceBuf corr[2], M[2];        // the two correspondence buffers (original target index / Mahalanobis matrix per source point), chosen by the state's parity
        pcr::DeviceBuf d2;                   // pcr_gicp_linearize: the correspondences' float distances
    } gi;

    // LIORF work memory (liorf_host.hip).  The target is h->grid (every finite point, for the 5-NN) over the handle's own copy of the points (tgt_stage);
    // the rows of a launch go to vg_partials, the scan kept for pcr_fitness() to fit_src.
    struct Liorf {
        pcr::DeviceBuf ctl;                  // two LiorfCtl: the state of the device-resident loop, by launch parity
        pcr::host::Mapped<pcr::LiorfOut> out;    // its result and progress word
        pcr::DeviceBuf kept, coeff, trace;   // pcr_liorf_linearize's per-point outputs; the per-iteration trace (pcr_params.record_trace)
        // the last alignment, for pcr_liorf_result
        bool have_result = false;
        float six[6] = {0, 0, 0, 0, 0, 0};
        int degenerate = 0;
        long long rows_last = 0;
    } lf;

    // region of interest of a target prepared for one scan (RoiView): two marking buffers used alternately, the dilated mask, the escape counter
    // (vgicp_host.hip: roi_enqueue, roi_view)
    struct Roi {
        pcr::DeviceBuf mark[2], tmp, mask, esc;
        int idx = 0, mshift = 0;
        uint64_t cells_seen = 0;     // cell count of the lattice the mark buffers were last used with (a change clears them in full)
    } roi;
    bool roi_on = false;             // the target structures the handle holds cover only the region of the scan they were prepared for (capi, vgicp, ndt)
    long long roi_repeats = 0;       // calls that left the region and were repeated on the whole target (vgicp, ndt; capi: pcr_get_stats)
    pcr::BlobStore blob;             // the optimiser's initial state as a rider of the region's mark pass (pcr_internal.h: BlobStore) (ndt fills it, roi_enqueue launches it)
    bool blob_pending = false;       //   filled in by this call and not launched yet (ndt, vgicp: roi_enqueue)
    bool blob_stored = false;        //   launched by this call: run_ndt needs no launch of its own for it

    // NDT work memory (ndt_host.hip)
    struct Nd {
        pcr::DeviceBuf slot, vox, count, list, partials;
        pcr::host::Mapped<double> out48;     // 48 doubles written by ndt_sum_partials_kernel
        pcr::DeviceBuf ctl;                  // NdtCtl: the device-resident optimiser's state
        pcr::DeviceBuf sums;                 // sharded device loop: the 48 sums of a pass, all-reduced in place
        pcr::host::Mapped<pcr::NdtOut> out;  // its result and progress word
        int count_idx = 0;
        int iters = 0, deriv = 0, hess = 0;
        double score = 0;
    } nd;
    bool nd_grid_checked = false, nd_grid_bad = false, nd_grid_empty = false;      // the device loop reported the state of the index header with its result (ndt: run_ndt writes, ndt_scan2map reads)
    uint64_t nd_grid_cells = 0;

    // the voxel filter (voxel_host.hip)
    struct Vf {
        pcr::GridIndex grid;             // pcl::VoxelGrid lattice of the cloud being down-sampled (pcr_voxel_filter)
        pcr::DeviceBuf in, out, head, sums, count;
        struct Job { const float* d_pts; size_t n, sf; double leaf; float* d_out; size_t cap; } job = {};      // the filter that is queued (vf_enqueue / vf_settle)
        bool inflight = false; size_t inflight_n = 0;      // pcr_voxel_filter_begin has queued a filter that pcr_voxel_filter_end has not collected
        char* ret = nullptr;             // page-locked: what the voxel filter's last block reports (VfResult: the voxel count + the index header's verdict)
    } vf;

    // the sparse voxel filters (voxel_sparse_host.hip): buffers kept between calls, all sized by the number of points
    struct Vs {
        pcr::DeviceBuf in, out, hdr, key[2], row[2], hist, cnt, first, lead, tile;
        pcr::host::Mapped<pcr::VsResult> ret;      // what the last launch reports (the call's one synchronisation reads it)
        bool have_order = false;         // the last call sorted something that pcr_voxel_sparse_order can hand out
        size_t order_n = 0; int order_buf = 0;
    } vs;

    // pcr_deskew (deskew_host.hip): a host scan and its packed times on their way in, the output of a call that returns it to the host, the control
    // block (the three counts, then the table), and the counts as the call's one synchronisation reads them
    struct Dsk {
        pcr::DeviceBuf in, times, out, ctl;
        pcr::host::Mapped<unsigned long long> ret;
    } dsk;

    // scores of many poses and exact queries on the kept target (query_host.hip)
    struct Query {
        pcr::DeviceBuf rl_poses, rl_part, rl_out, rl_src;   // pcr_fitness_batch: the poses in float, the [pose][chunk] partials, the sums; pcr_relocalize: its staged host source
        pcr::DeviceBuf idx, d2, idx2, d22, counts, offsets;      // pcr_knn / pcr_radius_search: results (radius, sorted: filled into one pair, sorted into the other), counts, offsets
        // the sparse index of the kept target (sparse_index.hip), built by the first query that needs it and dropped with the target (drop_query_index):
        // the keys and the points in key order, exactly 24 bytes per row of the target; what its build reported
        struct Sparse {
            pcr::DeviceBuf keys, pts;
            bool valid = false;
            pcr::sw::View view = {};
            pcr::host::Mapped<pcr::SiResult> ret;
        } sparse;
        int last_kind = -1;              // the index that answered the last query (PCR_QUERY_INDEX_DENSE / _SPARSE), -1: none since the target was set
        size_t last_points = 0, last_bytes = 0;
    } q;

    // multi-GPU: the tile of the map this rank holds (set by comm: pcr_set_shard / pcr_set_query_tile; read by loam, vgicp, ndt, query)
    int use_tile = 0;
    double tile_lo[3] = {0, 0, 0}, tile_hi[3] = {0, 0, 0};
    bool have_halo = false;          // pcr_set_shard: the target holds every map point inside [tile_lo - halo, tile_hi + halo)
    double halo = 0.0;
    // multi-GPU: the transport between the ranks (comm_host.hip).  The drivers of loam, vgicp and ndt hand `peer` and the next `peer_seq` to
    // their exchange launches and choose their loop by which transport is set.
    struct Comm {
        void* rccl = nullptr;            // RCCL communicator (pcr_comm_init)
        // peer exchange (pcr_comm_init_peer): this rank's receive buffer (fine-grained HBM, exported over IPC), every rank's as mapped here
        double* peer_own = nullptr;
        bool peer_on = false;
        bool peer_exported = false;      // pcr_comm_peer_export has cleared the receive buffer for a session that pcr_comm_init_peer has not opened yet
        bool peer_broken = false;        // an exchange of the session timed out: the ranks' sequence numbers no longer agree, every further exchange is refused
        pcr::host::Mapped<int32_t> peer_status;     // set by a kernel whose exchange timed out
        pcr::PeerComm peer{};
        double peer_seq = 0.0;
        pcr_allreduce_fn host_ar = nullptr;     // or the caller's collective (pcr_comm_init_host)
        void* host_ar_user = nullptr;
        int nranks = 1, rank = 0;
        pcr::DeviceBuf ar_stage;         // RCCL: staging of the 48 doubles the host-driven optimisers exchange
    } comm;

    // timing (capi: prof_begin / prof_end / read_call_times; the drivers record into it)
    hipEvent_t ev_start = nullptr, ev_index = nullptr, ev_end = nullptr;
    std::vector<hipEvent_t> ev_kernel;      // loam, ndt: a pair per launch timed on its own
    // profiling passes (pcr_set_profile 2) of NDT / VGICP: counters the kernels add to ([0] target points with a covariance, [16] voxels,
    // [32] / [48] (point, voxel) pairs of gradient-only / Hessian passes), events of the covariance kernels ([0..1] target, [2..7] scan's search)
    pcr::DeviceBuf prof_count;
    hipEvent_t ev_cov[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // vgicp records, capi reads
    bool ev_cov_tgt_used = false, ev_cov_src_used = false;
    int nd_prof_launches = 0;        // ndt records, capi reads
    pcr_stats stats;                 // every driver
};

namespace pcr {
namespace host {

#define H_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { h->err = std::string(#x) + ": " + hipGetErrorString(_e); return 1; } } while (0)

// inside a loop that has launches reading the caller's buffers queued ahead of the device: an error must not return before they drained
#define H_TRY_DRAIN(x) do { hipError_t _e = (x); if (_e != hipSuccess) { h->err = std::string(#x) + ": " + hipGetErrorString(_e); (void)hipStreamSynchronize(h->stream); return 1; } } while (0)

// what pcr_last_error(NULL) returns: the message of a call that has no handle to leave it in (capi.hip)
extern thread_local std::string g_create_error;

inline int fail(pcr_handle* h, const std::string& msg) { h->err = msg; return 1; }
inline bool sharded(const pcr_handle* h) { return h->comm.rccl != nullptr || h->comm.host_ar != nullptr || h->comm.peer_on; }
// pcr_params.vgicp_search beyond DIRECT1 on a vgicp handle that has a tile or a communicator: a neighbour voxel may belong to another rank's tile, and no
// halo rule serves that yet.  The refusal of pcr_set_shard, pcr_comm_init* and pcr_set_params, naming the setting; nullptr when there is nothing to refuse.
inline const char* vgicp_search_shard_refusal(const pcr_handle* h, int search, bool becoming_sharded) {
    if (h->method != kVgicp || search == PCR_VGICP_DIRECT1 || !(becoming_sharded || sharded(h) || h->use_tile)) return nullptr;
    return search == PCR_VGICP_DIRECT7
        ? "vgicp: pcr_params.vgicp_search = 1 (DIRECT7) is not served on a sharded handle (a neighbour voxel may belong to another rank's tile); use 2 (DIRECT1)"
        : "vgicp: pcr_params.vgicp_search = 0 (DIRECT27) is not served on a sharded handle (a neighbour voxel may belong to another rank's tile); use 2 (DIRECT1)";
}
// profiling passes: the counters the kernels add to, or nullptr
inline uint32_t* prof_counters(const pcr_handle* h) { return (h->profile >= 2 && h->prof_count.p) ? h->prof_count.as<uint32_t>() : nullptr; }
// Whatever the scan's side has in flight on the side stream is waited for: nothing stays in flight behind the caller's back.
inline hipError_t side_drain(pcr_handle* h) {
    if (!h->side_pending) return hipSuccess;
    h->side_pending = false;
    return hipEventSynchronize(h->ev_side_done);
}

// The scan a target is being prepared for (pcr_scan2map of an unsharded handle), or nullptr: everything is prepared.
struct RoiScan { const float* d_src; size_t n_src, stride_floats; const double* pose; };

// ---- capi.hip ----
// What the entry points dispatch on, one row per Method (the table itself: capi.hip).  The functions of a row live in the method's own unit.
typedef int Scan2MapFn(pcr_handle* h, const float* d_src, size_t n_src, const float* d_dst, size_t n_dst, size_t stride_floats, double pose[16], int* converged);
typedef int PrepareTargetFn(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats);
typedef int AlignFn(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged);
typedef bool TargetFromChangedFn(const pcr_params& old_p, const pcr_params& new_p);
struct MethodOps {
    const char* name;                // pcr_create's lookup, the prefix of the refusal of a sharded target
    bool shardable;                  // pcr_set_shard, pcr_set_query_tile and pcr_comm_init* serve the method
    bool passes_profiled;            // pcr_scan2map starts the profiling passes (prof_begin) and the method ends the call with end_timed_call
    bool scores_kept_scan;           // pcr_fitness() evaluates the scan the last alignment kept, on demand; else it returns 0
    double fit_max_sq, fit_none;     // ... the score's gate and its value when no point counts
    Scan2MapFn* scan2map;            // pcr_scan2map: the target prepared for this scan and the scan aligned to it (both clouds in HBM, ev_start recorded)
    PrepareTargetFn* prepare_target; // a target that is kept, from points in HBM that outlive it: pcr_set_target, a sub-map, ensure_full_target
    AlignFn* align;                  // pcr_align, once the handle has a target
    TargetFromChangedFn* target_from_changed;      // pcr_set_params: what the prepared target was derived from has changed
};
Scan2MapFn loam_scan2map, ndt_scan2map, vgicp_scan2map, gicp_scan2map, liorf_scan2map;
PrepareTargetFn loam_prepare_target, ndt_kept_target, vgicp_kept_target, gicp_kept_target, liorf_prepare_target;
AlignFn loam_align, run_ndt, vgicp_align, gicp_align, run_liorf;
TargetFromChangedFn loam_target_from_changed, ndt_target_from_changed, vgicp_target_from_changed, gicp_target_from_changed, liorf_target_from_changed;
const MethodOps& ops(const pcr_handle* h);
// the handle holds a target prepared in full by prepare_target (pcr_scan2map_submap: nothing to rebuild while the map's generation lasts)
inline bool target_prepared(const pcr_handle* h) { return h->method == kLoam ? h->grid.valid && !h->clamp.use : h->target_ready; }
int read_call_times(pcr_handle* h);
int end_timed_call(pcr_handle* h);
int ensure_full_target(pcr_handle* h);

// ---- staging_host.hip ----
int stage_host(pcr_handle* h, DeviceBuf* buf, const void* src, size_t n, size_t stride_bytes, const float** out, bool whole_records = false);
int check_stride(pcr_handle* h, size_t stride_bytes);
int set_device(pcr_handle* h);
int ensure_out32(pcr_handle* h);
int wait_result(pcr_handle* h, const double* flag_word, double seq);
void pin_forget_stream(hipStream_t stream);

// ---- comm_host.hip ----
int ranks_allreduce(pcr_handle* h, double* v, int n, int op = 0);
int rccl_sum(pcr_handle* h, void* d_buf, size_t n);
int agree_prepared(pcr_handle* h, int rc_local);
void peer_close(pcr_handle* h);
int peer_check(pcr_handle* h);
void comm_release(pcr_handle* h);
void shard_extent(const pcr_handle* h, double ext_lo[3], double ext_hi[3]);
// the halo an ndt tile needs under pcr_params.ndt_search at this resolution, and the refusal that names the setting (pcr_set_shard, pcr_set_params)
double ndt_halo_need(int search, double res);
std::string ndt_halo_message(int search, double need);

// ---- loam_host.hip ----
int build_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats);
int set_clamp_from_scan(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16]);
int set_clamp_from_target_sample(pcr_handle* h, bool room = false);
int settle_loam_index(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, const double* pose);
int run_loam(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged, bool index_timed);

// ---- vgicp_host.hip ----
int settle_grid(pcr_handle* h, GridIndex& g, const float* d_pts, size_t n, size_t stride_floats, double cell, int pcl_mode = 0, const ClampBox* clamp = nullptr);
int roi_enqueue(pcr_handle* h, const RoiScan& scan, double cell, double base_m, RoiView* view);
RoiView roi_view(const pcr_handle* h);
int vgicp_source_mark(pcr_handle* h);
int vgicp_source_enqueue(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, bool marked = false, std::string* errp = nullptr);
int vgicp_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, const RoiScan* roi_scan = nullptr, bool keep_clamp = false,
                         const std::function<int()>* before_wait = nullptr);
int vgicp_align_recut(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged);
// pcr_align of vgicp and gicp: the scan's side queued unless pcr_scan2map_submap has queued it, `run`, the side stream drained
int align_beside_scan_side(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged, AlignFn* run);

// What settle_cov_levels does beyond building and sizing the levels
struct CovSettle {
    double shift0 = 0.0;                  // shift of the fine level's lattice, in cells
    GridHeader* hdr0_out = nullptr;       // where the fine level's header goes, with its density figure
    bool may_cut = false;                 // a box no dense table can hold is cut to the bulk of the cloud (h->clamp)
    double ahead_cell = 0.0;              // a one-level cloud: the cell of its covariance grid, built ahead in l1 beside the fine level; 0: none
    bool* ahead_ok = nullptr;             // ... whether that grid stands
    // after_ahead (with a grid built ahead only): what the caller would enqueue once the headers have been read, enqueued BEFORE they are -- the
    // host waits for the headers alone (an event behind their copies) while the device goes on; *after_clean tells whether what was enqueued
    // stands (first attempt, nothing stale or overflowing, the grid built ahead usable).  Kernels queued that way see the flags in the headers
    // and leave early; whatever they wrote is written again by the caller.
    const std::function<int()>* after_ahead = nullptr;
    bool* after_clean = nullptr;
    const std::function<int()>* before_wait = nullptr;      // what the caller wants queued on OTHER streams while the host waits for the headers
    // scan_levels: the levels of a SCAN (the source of an alignment that did not come through vgicp_source_enqueue: pcr_set_target + pcr_align,
    // pcr_vgicp_covariances, the redo path): built like vgicp_source_enqueue builds them -- one-level path, no hints: one scan's box and tile
    // layout do not hold the next (walls at other distances; measured there: every hint failed and the redo cost 0.9 ms)
    bool scan_levels = false;
    // filter0: the fine level may index the points of a region only (BuildFilter: possible when this build reuses the header and the tile layout of
    // an earlier full build of the level -- build() decides and says so in filter0->applied)
    BuildFilter* filter0 = nullptr;
    bool* untabulatable = nullptr;        // set when the call fails because a level's box needs more cells than a dense table can have and may_cut is off
};
// the fine index plus the coarse ones of the covariance search, settled with one round trip (gicp prepares its target with it too)
int settle_cov_levels(pcr_handle* h, GridIndex& g, GridIndex& l1, GridIndex& l2, const float* d_pts, size_t n, size_t stride_floats, double cell,
                      const CovSettle& opt);
int cov_levels(size_t n);      // index levels of a cloud's covariance search: 2 for a scan-sized cloud, 1 for a map-sized one
// the scan's covariances (vg.src_cov6) ready on return, ordered before whatever the main stream runs next: collected from the side stream, or computed here
int vgicp_source_settle(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats);

// ---- gicp_host.hip ----
int gicp_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, const std::function<int()>* before_wait = nullptr);
int run_gicp(pcr_handle* h, const float* d_src, size_t n_src, size_t stride_floats, double pose[16], int* converged);
// vgicp and gicp: the methods whose scan side (its index levels and covariances) runs on the side stream
inline bool vgicp_family(const pcr_handle* h) { return h->method == kVgicp || h->method == kGicp; }

// ---- liorf_host.hip ----
// the liorf_* field of pcr_params that is out of range, named; nullptr when all are in range (pcr_create, pcr_set_params: every handle)
const char* liorf_params_out_of_range(const pcr_params& p);

// ---- ndt_host.hip ----
int ndt_prepare_target(pcr_handle* h, const float* d_dst, size_t n_dst, size_t stride_floats, bool deferred = false, const RoiScan* roi_scan = nullptr);
int ndt_ride_initial_state(pcr_handle* h, const double pose[16]);

// ---- fitness_host.hip: the scan an alignment keeps for pcr_fitness() (the methods whose row says scores_kept_scan) ----
void drop_fitness_state(pcr_handle* h);
bool fitness_scan_kept(pcr_handle* h, const float* d_src);
int keep_scan_for_fitness(pcr_handle* h, const float* d_src, size_t n, size_t stride_floats, bool kept);
void arm_fitness(pcr_handle* h, const double pose[16], size_t n, size_t stride_floats);

// ---- query_host.hip ----
std::string cut_fitness_message(double n);
// the kept target has changed or is gone: the sparse index built from it goes too (capi: every entry point that sets or drops a target)
void drop_query_index(pcr_handle* h);
// pcr_params.query_index = SPARSE governs this handle's scores: always the sparse index (not a sharded handle, not one with a query tile)
inline bool scores_on_sparse(const pcr_handle* h) { return h->prm.query_index == PCR_QUERY_INDEX_SPARSE && !sharded(h) && !h->use_tile; }
// One pose scored on the sparse index of the kept target (built when the handle has none), the sums left in h->out32.host[0..2] as fitness_launch
// leaves them.  n_viol > 0: the dense kernel could not answer for that many points (a cut index) and this is the fall-back -- where the sparse
// index cannot be had either, the message is cut_fitness_message's followed by the index's own reason; n_viol = 0: the caller asked for the index.
int sparse_fitness_run(pcr_handle* h, const char* who, double n_viol, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16],
                       double max_sq);

// How a device-resident optimiser's passes (run_lsq, run_ndt) are queued ahead of the progress word of its result block
struct PaceRule {
    long first;       // passes queued before the first look
    long ahead;       // passes kept queued beyond those the device has consumed
    long refill;      // passes queued after a forced synchronisation
    // A peer-exchange session: every rank must queue the same number of launches whatever it happens to see when, or the ranks'
    // sequence numbers part and the next exchange waits out its timeout.  So never more than `ahead` beyond the passes consumed,
    // and exactly P + ahead once the loop has finished after P passes (the launches beyond the end exchange nothing and leave);
    // a profiler does not force a synchronisation, and the session is checked after one.
    bool peer;
};
// the rule of every loop over the peer exchange (run_ndt, run_vgicp): nothing before the first look, three launches ahead
static constexpr PaceRule kPeerPace{0, 3, 0, true};

// Queue the passes of call `seq` by `rule` -- launch(i) queues pass i -- until the device loop writes `seq` into out->seq.
// limit: the pass budget of the call; window_msg / budget_msg: the errors of a budget that exceeds the progress window, or
// that ran out.
template <class Out, class Launch>
int pace_passes(pcr_handle* h, const Out* out, double seq, long limit, const PaceRule& rule, const char* window_msg, const char* budget_msg,
                Launch&& launch) {
    if ((double)limit >= kProgressWindow) return fail(h, window_msg);
    const volatile double* f_seq = &out->seq;
    const volatile double* f_prog = &out->progress;
    const long cap = rule.peer ? limit + rule.ahead : limit;
    long enq = 0, spins = 0;
    for (; enq < rule.first; ++enq) H_TRY_DRAIN(launch(enq));
    while (*f_seq != seq) {
        const double pr = *f_prog;
        const long consumed = (pr >= seq * kProgressWindow && pr < (seq + 1.0) * kProgressWindow) ? (long)(pr - seq * kProgressWindow) : 0;
        if (enq - consumed < rule.ahead && enq < cap) { H_TRY_DRAIN(launch(enq)); ++enq; continue; }
        __builtin_ia32_pause();
        if (++spins > 400000 || (!rule.peer && h->profile != 0)) {      // a slow device (or a profiler): wait for what is queued, then look again
            H_TRY(hipStreamSynchronize(h->stream));
            if (*f_seq == seq) break;
            if (rule.peer && peer_check(h)) return 1;
            if (enq >= cap) return fail(h, budget_msg);      // (stream just drained)
            spins = 0;
            for (long k = 0; k < rule.refill && enq < cap; ++k, ++enq) H_TRY_DRAIN(launch(enq));
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (rule.peer) {
        for (const long want = (long)out->passes + rule.ahead; enq < want; ++enq) H_TRY_DRAIN(launch(enq));
        if (peer_check(h)) return 1;
    }
    return 0;
}

}  // namespace host
}  // namespace pcr
