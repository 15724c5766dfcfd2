/*
 * pcr_hip.h -- C ABI of the MI355X-native scan-to-map registration library
 * (libpcr_hip.so).  Plain pointers and sizes only; no C++/torch types.
 *
 * It is the drop-in boundary for the reference's registration plugin
 *   PCR::PointCloudRegister::scan2Map(const PC_cPtr& src, const PC_cPtr& dst, pose_t& res)
 *   (reference PCR/include/PCR/PointCloudRegister.hpp:12-38)
 * and its three implementations selected by the config key frontend.pcr
 *   "loam"  -> PCR::LoamRegister   (PCR/src/LoamRegister.cpp:99-223)
 *   "ndt"   -> PCR::NdtRegister    (PCR/src/NdtRegister.cpp:21-31)
 *   "vgicp" -> PCR::VgicpRegister  (PCR/src/VgicpRegister.cpp:30-45)
 *   (factory: frontend/src/LidarOdometry.cpp:44-54).
 * INTEGRATION.md shows the reference-side adapter class that binds these entry
 * points; simpleslam_amd/host/PCR mirrors the reference classes without PCL/Eigen.
 *
 * Conventions
 *   - A point is `stride_bytes` bytes whose first 12 are float x,y,z.
 *     stride 32 = pcl::PointXYZI (reference common/types/basic.hpp:16), 16 = float4.
 *   - A pose is 16 doubles, column-major 4x4 (Eigen::Isometry3d::matrix().data(),
 *     reference common/types/basic.hpp:19); in = initial guess, out = refined.
 *   - Every call returns 0 on success, nonzero on error; pcr_last_error() then
 *     describes it.  Nothing throws across this boundary.  A handle serves one
 *     caller at a time; distinct handles are independent (own stream and buffers).
 */
#ifndef PCR_HIP_H
#define PCR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcr_handle pcr_handle;

/* Defaults (pcr_default_params) are the reference's constants; see SURVEY.md App. A. */
typedef struct pcr_params {
    uint32_t struct_size;      /* sizeof(pcr_params), set by pcr_default_params */
    int32_t device;            /* HIP device ordinal; -1 = current device */

    /* LOAM -- PCR/include/PCR/LoamRegister.hpp:30-40 */
    int32_t loam_iters;        /* 8   iteration cap (LoamRegister.hpp:40) */
    int32_t loam_early_exit;   /* 1   stop when the step is small (LoamRegister.cpp:202-206) */
    double loam_knn_max_sq;    /* 1.0 gate on the SQUARED 5th-neighbour distance (LoamRegister.cpp:59) */
    double loam_plane_thresh;  /* 0.2 plane validity, times |x| (LoamRegister.cpp:39) */
    double loam_point_thresh;  /* 0.1 weight gate (LoamRegister.cpp:151) */
    double loam_pos_conv;      /* 5e-3 (LoamRegister.hpp:37) */
    double loam_rot_conv;      /* 5e-3 (LoamRegister.hpp:38) */

    /* NDT -- PCR/src/NdtRegister.cpp:12-13, third_parties/pclomp/src/ndt_omp_impl.hpp:50-51,71-72 */
    double ndt_resolution;     /* 1.0 */
    double ndt_step_size;      /* 0.1 */
    double ndt_outlier_ratio;  /* 0.55 */
    double ndt_trans_eps;      /* 0.1 */
    int32_t ndt_max_iters;     /* 35 */
    int32_t ndt_min_points;    /* 6 points per voxel (pclomp/voxel_grid_covariance_omp.h:210) */

    /* pclomp::NormalDistributionsTransform::setNeighborhoodSearchMethod (third_parties/pclomp/src/pclomp/ndt_omp.h:52-57,189-191): which voxels
     * a transformed scan point is differentiated against.  Read by ndt handles ONLY (every other handle accepts any served value and ignores
     * it).  A value outside 0..3, and PCR_NDT_KDTREE, are refused by pcr_create and pcr_set_params.  A change through pcr_set_params KEEPS
     * the prepared target -- the voxel Gaussians do not depend on the neighbourhood -- and checks the halo of a sharded handle again. */
    int32_t ndt_search;        /* PCR_NDT_*, default PCR_NDT_DIRECT7 (PCR/src/NdtRegister.cpp:13).  With c = floor(p / resolution) per axis, in float, a
                                *    cell c + d counts when it lies inside the target's lattice box and its voxel was kept (>= ndt_min_points points, the
                                *    eigenvalue and inverse tests passed) -- voxel_grid_covariance_omp_impl.hpp:374-441:
                                *    DIRECT1 d = 0; DIRECT7 d = 0 and the six face cells; DIRECT26 the 26 cells of the 3 x 3 x 3 block around c, c itself
                                *    EXCLUDED (pcl::getAllNeighborCellIndices).  The float derivative pass, its line-search variant and the double
                                *    computeHessian pass all follow it (ndt_omp_impl.hpp:233-246, :572-585).
                                *    KDTREE is not served, for three reasons: the reference searches FLANN over the voxel centroids, float running sums
                                *    in input order (voxel_grid_covariance_omp_impl.hpp:289), so its result depends on the order of the target's rows,
                                *    which nothing in this library does; voxels that failed the covariance tests (:337-341, :360-364) stay in that
                                *    centroid cloud and radiusSearch returns them without an nr_points test (voxel_grid_covariance_omp.h:489-503), so
                                *    the reference differentiates against whatever their icov_ holds; and FLANN is not available to pin either down. */

    /* VGICP -- PCR/src/VgicpRegister.cpp:13, third_parties/pclomp/src/fast_vgicp_impl.hpp:22-24,
     * fast_gicp_impl.hpp:16-20, lsq_registration_impl.hpp:11-18 */
    double vgicp_resolution;   /* 1.0 */
    int32_t vgicp_k_corr;      /* 20 neighbours for the covariances */
    int32_t vgicp_max_iters;   /* 64 */
    int32_t vgicp_lm_inner;    /* 10 */
    double vgicp_rot_eps;      /* 2e-3 */
    double vgicp_trans_eps;    /* 5e-4 */
    double vgicp_lm_init_scale;/* 1e-9 */
    /* fast_gicp::FastVGICP::setNeighborSearchMethod (third_parties/pclomp/src/pclomp/gicp_settings.hpp:8, fast_vgicp_impl.hpp:73-116,
     * pclomp/fast_vgicp_voxel.hpp:10-44): which voxels a transformed scan point is paired with.  Read by vgicp handles ONLY (gicp, ndt and loam
     * handles accept any served value and ignore it).  A value outside 0..3, and PCR_VGICP_DIRECT_RADIUS (the reference marks it "only
     * VGICP_CUDA"), are refused by pcr_create and pcr_set_params.  A change through pcr_set_params KEEPS the prepared target -- the voxels do
     * not depend on the neighbourhood -- and the correspondence buffers are sized again by the next call.  DIRECT7 and DIRECT27 are refused on
     * a sharded handle (pcr_set_shard, pcr_comm_init*, pcr_set_params): a neighbour voxel may belong to another rank's tile. */
    int32_t vgicp_search;      /* PCR_VGICP_*, default PCR_VGICP_DIRECT1 (fast_vgicp_impl.hpp:23).  With c = floor(T p / resolution - 0.5) per axis, in
                                *    double, a PAIR (p, voxel) exists for every offset d of the setting's table for which the voxel c + d exists in the
                                *    target; a cell outside the target's lattice box holds no voxel, and c + d is tested per axis, so a point whose own cell
                                *    lies one layer outside the box still reaches the box's outer voxels under DIRECT7 / DIRECT27.
                                *    DIRECT1 d = 0; DIRECT7 d = 0, then +x -x +y -y +z -z (fast_vgicp_voxel.hpp:21-29); DIRECT27 all of {-1, 0, 1}^3 with x
                                *    outermost and z fastest, the centre INCLUDED (:31-41; unlike NDT's DIRECT26).
                                *    Every pair is a term of H, b and the error exactly as the single pair is: M = (C_B + T C_A T^T)^-1, weight
                                *    sqrt(num_points), J = [skew(T p) | -I]; compute_error at an LM trial pose reuses the pairs and the M of the last
                                *    linearisation (fast_vgicp_impl.hpp:183-204).  A point's pairs are added in table order, then the fixed-order
                                *    reduction: no atomics, the device loop equals the host loop and a repeated call gives the same bits. */

    int32_t record_trace;      /* 1: keep per-iteration normal equations for pcr_get_trace */

    /* ---- switches (all 0 by default; none of them changes a result except where noted).  The library reads NO environment
     * variable: what used to be PCR_* variables and pcr_params.reserved[] are these fields, or were removed. ---- */
    int32_t index_no_hints;    /* 1: every target index is built from scratch -- fresh bounding box, no tile layout taken over from the
                                *    previous build of this handle (three build launches instead of two; no state crosses calls) */
    int32_t ndt_evaluate_repeats; /* 1: NDT: every request of the line search becomes an evaluation pass, also one at the point just
                                *    evaluated (what the reference does; by default such a request is answered from the sums already
                                *    held -- same numbers, csrc/ndt_opt.h) */
    int32_t loam_disable_cache;/* 1: LOAM: no temporal-coherence neighbour cache, every iteration searches (same result bit for bit) */
    int32_t record_timeline;   /* 1: LOAM: record the in-kernel timeline of every launch (pcr_get_timeline) */
    int32_t loam_coresident;   /* 1: LOAM: the two-waves-per-SIMD variant of the iterate kernel -- ~3 % slower for one handle, ~25 % more
                                *    scans/s when several handles register scans concurrently on one GPU (their blocks share the CUs) */
    int32_t loam_clamp_margin_mm; /* != 0: LOAM: first margin, in millimetres, of the region a target too sparse for the dense index is
                                *    cut to around the scan (default 10 m; it grows whenever a query reaches a cut face).  Negative values cut
                                *    into the scan's own box: a test hook that makes the widening path reachable with ordinary clouds */
    int32_t full_target;       /* 1: NDT, VGICP: pcr_scan2map prepares the WHOLE target (every covariance, every voxel Gaussian), as the
                                *    reference does, instead of only the region the scan can reach (same result: a call whose pose leaves
                                *    the region is repeated on the whole target anyway) */
    int32_t host_optimiser;    /* 1: NDT, VGICP: drive the optimiser from the host (one round trip per evaluation pass) instead of on the
                                *    device; the path handles sharded over a host-supplied collective always take.  Same state machines
                                *    (csrc/ndt_opt.h, csrc/vgicp_opt.h), same result to rounding */
    int32_t host_copy_xyz;     /* 1: of HOST clouds whose records are wider than 16 bytes (pcl::PointXYZI: 32) only the first 16 bytes of every record are
                                *    uploaded (a pitched hipMemcpy2DAsync into a staging area of the same stride; registration reads x, y, z and nothing
                                *    else).  Off by default: measured on MI355X / ROCm 7.2 the pitched copy of a 1 M-point map takes 3.5 ms where the
                                *    verbatim copy of twice the bytes takes 0.6 ms (profiles/r04_notes.md) */
    int32_t query_index;       /* PCR_QUERY_INDEX_*: the index pcr_knn and pcr_radius_search answer from (no other call reads it).  AUTO (0, the default): the
                                *    dense cell table whenever it holds every point, the sparse index (sorted cell keys, memory by the points alone) for a
                                *    target whose box no dense table can hold.  SPARSE (1): always the sparse index.  Same answers bit for bit.  A value
                                *    out of range is refused by pcr_create and pcr_set_params */

    /* LIORF -- test/comp/liorf_scan2map.cpp (LioScan2map: LIO-SAM's surface scan-to-map).  Read by liorf handles only; every handle refuses a
     * value out of range, by name (pcr_create, pcr_set_params).  (The block stands in front of the struct's last three fields, whose place
     * at the end a test pins, as ndt_search and vgicp_search stand with their methods.)  The thresholds are the file's `double` literals: a float quantity is widened
     * and compared in double, as the file's expressions do. */
    int32_t liorf_iters;          /* 30   iteration cap (:392); >= 0 */
    int32_t liorf_file_row;       /* 0    the pitch entry of a row is the derivative of the residual; 1: the file's own line 310, which has
                                   *      sin(pitch) where the derivative has cos(pitch) in one term -- for a comparison with the program as written */
    double liorf_knn_max_sq;      /* 1.0  gate on the squared 5th-neighbour distance, strict '<' (:186); > 0 */
    double liorf_plane_thresh;    /* 0.2  a plane is invalid when one of its five points lies farther from it, strict '>' (:207); > 0 */
    double liorf_point_thresh;    /* 0.1  a point is kept when its weight s exceeds this, strict '>' (:224); finite */
    int32_t liorf_min_rows;       /* 50   fewer kept points: the pose is left alone (:268); >= 0 */
    int32_t liorf_min_scan;       /* 30   nothing happens unless the scan has MORE points than this (:388); >= 0 */
    double liorf_rot_conv_deg;    /* 0.05 converged: the angle step, in degrees, below this ... (:379); >= 0 */
    double liorf_trans_conv_cm;   /* 0.05 ... and the translation step, in centimetres, below this; >= 0 */
    double liorf_degenerate_eig;  /* 100  iteration 0: isDegenerate when the smallest eigenvalue of AtA is below this (:342); finite */

    /* GICP -- third_parties/pclomp/src/fast_gicp_impl.hpp:16-20.  A gicp handle also reads vgicp_resolution (the cell of its target index: it
     * decides how many candidates a search visits, never a result), vgicp_k_corr, vgicp_max_iters, vgicp_lm_inner, vgicp_rot_eps,
     * vgicp_trans_eps, vgicp_lm_init_scale, host_optimiser and index_no_hints. */
    double gicp_max_corr_dist; /* FLT_MAX  a correspondence needs a squared distance below (float)d * (float)d, formed in float: +inf by default
                                *    (fast_gicp_impl.hpp:18,136); VgicpRegister::initForLC sets 150 */

    /* fast_gicp's two public settings (third_parties/pclomp/src/pclomp/gicp_settings.hpp:6,10; FastGICP::setRegularizationMethod,
     * FastVGICP::setVoxelAccumulationMode).  A value outside the range is refused by pcr_create and pcr_set_params; a change through
     * pcr_set_params drops the prepared target. */
    int32_t vgicp_regularization; /* PCR_REG_*, default PCR_REG_PLANE (fast_gicp_impl.hpp:20).  vgicp and gicp handles, the source's covariances and the
                                *    target's alike (fast_gicp_impl.hpp:263-293), on the scatter C of the 20 neighbours with eigenvalues w, eigenvectors V:
                                *    NONE C itself; MIN_EIG V diag(max(w, 1e-3)) V^T; NORMALIZED_MIN_EIG V diag(max(w / w_max, 1e-3)) V^T;
                                *    PLANE V diag(1, 1, 1e-3) V^T; FROBENIUS (C_inv / |C_inv|_F)^-1 with C_inv = (C + 1e-3 I)^-1 */
    int32_t vgicp_voxel_mode;  /* PCR_VOXEL_*, default PCR_VOXEL_ADDITIVE (fast_vgicp_impl.hpp:24).  vgicp handles only (a gicp handle has no voxels and
                                *    ignores it).  ADDITIVE: mean of the points, mean of their covariances.  MULTIPLICATIVE
                                *    (fast_vgicp_voxel.hpp:79-103): cov = (sum C_i^-1)^-1, mean = cov * sum C_i^-1 p_i.  ADDITIVE_WEIGHTED is ADDITIVE
                                *    bit for bit: the vendored fast_gicp constructs the same AdditiveGaussianVoxel for both (fast_vgicp_voxel.hpp:138-141)
                                *    and weighs a correspondence by sqrt(num_points) in every mode (fast_vgicp_impl.hpp:149,199) */
} pcr_params;

/* pcr_params.ndt_search: pclomp::NeighborSearchMethod, in the enum's order */
#define PCR_NDT_KDTREE 0
#define PCR_NDT_DIRECT26 1
#define PCR_NDT_DIRECT7 2
#define PCR_NDT_DIRECT1 3

/* pcr_params.vgicp_search: fast_gicp::NeighborSearchMethod, in the enum's order */
#define PCR_VGICP_DIRECT27 0
#define PCR_VGICP_DIRECT7 1
#define PCR_VGICP_DIRECT1 2
#define PCR_VGICP_DIRECT_RADIUS 3

/* pcr_params.vgicp_regularization: fast_gicp::RegularizationMethod, in the enum's order */
#define PCR_REG_NONE 0
#define PCR_REG_MIN_EIG 1
#define PCR_REG_NORMALIZED_MIN_EIG 2
#define PCR_REG_PLANE 3
#define PCR_REG_FROBENIUS 4
/* pcr_params.vgicp_voxel_mode: fast_gicp::VoxelAccumulationMode, in the enum's order */
#define PCR_VOXEL_ADDITIVE 0
#define PCR_VOXEL_ADDITIVE_WEIGHTED 1
#define PCR_VOXEL_MULTIPLICATIVE 2

/* pcr_params.query_index, and the `kind` pcr_query_index_info reports */
#define PCR_QUERY_INDEX_AUTO 0
#define PCR_QUERY_INDEX_SPARSE 1
#define PCR_QUERY_INDEX_DENSE 0      /* pcr_query_index_info: the dense cell table answered */

/* Per-call device timings, from HIP events on the handle's stream. */
typedef struct pcr_stats {
    double total_ms;        /* whole call on the device timeline */
    double index_ms;        /* target index build (0 when the cached index was used) */
    double solve_ms;        /* all optimisation launches */
    double kernel_ms;       /* sum over the dominant kernel's launches (only with pcr_set_profile(h,2)) */
    int32_t kernel_launches;/* launches summed in kernel_ms */
    int32_t iterations;     /* linearisations performed */
    int64_t n_src, n_dst;
    int32_t attempts;       /* LOAM: passes over the iteration loop (> 1: the cell table grew, or a cut index was widened);
                             * NDT: evaluation passes the device loop launched -- fewer than kernel_launches (= the evaluations the
                             * reference makes) when repeated line-search evaluations were answered without a pass */
    int32_t target_builds;  /* pcr_scan2map_submap: times this handle has (re)built its target structures (one per sub-map generation) */
    int32_t region_repeats; /* NDT, VGICP pcr_scan2map: calls of this handle so far whose pose left the region the target had been prepared for and
                             * that were therefore repeated on the whole target (pcr_params.full_target) */
    int32_t region_index;   /* NDT pcr_scan2map: 1 when the last call's target index itself held only the points of the scan's region (possible once
                             * an earlier call of the handle has left its lattice and tile layout as hints), 0 when it held the whole cloud */
    /* Filled by a call made under pcr_set_profile(h, 2) only (events at the kernels' own begin and end, counters in the kernels): what the
     * last NDT / VGICP pcr_scan2map really processed, so that a roofline figure can be computed from the work done.
     *   VGICP: kernel_ms = the target's covariance kernel (vgicp_cov_kernel<false>), aux_kernel_ms = the three kernels of the scan's own
     *          covariance search (csrc/cov_search.hip), region_points / region_voxels = target points whose covariance was computed / voxels built
     *   NDT:   kernel_ms / kernel_launches = the evaluation launches of the device loop (ndt_pass_pro_kernel), pairs_grad / pairs_hess =
     *          (point, voxel) pairs evaluated by the gradient-only passes / by the passes that also accumulate the float Hessian */
    double aux_kernel_ms;
    int64_t region_points, region_voxels, pairs_grad, pairs_hess;
    /* the handle's last build of its target index: did it reuse the previous target's bounding box (header), and did it place its points by the
     * previous build's tile layout (both are hints that are checked on the device; a hint that failed shows as 0: the build was redone without it) */
    int32_t index_box_hint, index_layout_hint;
} pcr_stats;

void pcr_default_params(pcr_params* p);

/* method = "loam" | "ndt" | "vgicp" | "gicp" (frontend.pcr; "gicp" is fast_gicp::FastGICP, the point-wise class FastVGICP derives from, under
 * VgicpRegister's interface: every entry point a vgicp handle serves, the whole target prepared at every preparation; sharding -- pcr_set_shard,
 * pcr_set_query_tile, pcr_comm_init* -- and a target whose box no dense table can hold are refused) | "liorf" (LIO-SAM's surface scan-to-map,
 * the reference's test/comp/liorf_scan2map.cpp: see pcr_liorf_* below; the same two refusals).  NULL on failure; pcr_last_error(NULL)
 * then holds the reason (unknown method: the reference factory throws,
 * LidarOdometry.cpp:50-54).  p == NULL uses the defaults. */
pcr_handle* pcr_create(const char* method, const pcr_params* p);
void pcr_destroy(pcr_handle* h);
const char* pcr_last_error(const pcr_handle* h);

/* scan2Map with HOST buffers (what PCR::PointCloudRegister::scan2Map hands over:
 * src->points.data(), dst->points.data()).  The target index is rebuilt on every
 * call, as the reference does (LoamRegister.cpp:110).  *converged = isConverge. */
int pcr_scan2map(pcr_handle* h, const void* src, size_t n_src, const void* dst, size_t n_dst,
                 size_t stride_bytes, double pose_inout[16], int* converged);

/* Page-lock a host buffer that will be handed to pcr_scan2map / pcr_set_target / pcr_align (and the other entry points taking host
 * clouds) repeatedly -- e.g. the sub-map's point array between two MapManager updates: the upload then reads the caller's pages
 * directly (~55 GB/s over PCIe 5 x16) instead of going through the runtime's staging of pageable memory.  Explicit on purpose:
 * the registration holds for exactly the range [ptr, ptr + bytes) until pcr_host_unpin(ptr), which MUST precede freeing or
 * reallocating the buffer -- the library never keys anything on a pointer it merely remembers.  Process-wide, any
 * thread; the CONTENT is still copied on every call.  Errors: nonzero, message in pcr_last_error(NULL). */
int pcr_host_pin(const void* ptr, size_t bytes);
int pcr_host_unpin(const void* ptr);

/* Same with DEVICE-resident buffers (HBM pointers valid on the handle's device). */
int pcr_scan2map_device(pcr_handle* h, const void* d_src, size_t n_src, const void* d_dst, size_t n_dst,
                        size_t stride_bytes, double pose_inout[16], int* converged);

/* Static-map localisation (reference test/loc.cpp: one PCD map, many scans): build
 * the target index once, then align scans against it.  on_device != 0 marks the
 * buffers as HBM pointers.  The library copies what it keeps. */
int pcr_set_target(pcr_handle* h, const void* dst, size_t n_dst, size_t stride_bytes, int on_device);
int pcr_align(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device,
              double pose_inout[16], int* converged);
/* Drop the cached target (the reference caches by pointer identity and goes stale,
 * SURVEY.md F10; this library never keys on the pointer). */
int pcr_invalidate_target(pcr_handle* h);

/* PointCloudRegister::getFitnessScore (PointCloudRegister.hpp:34; VgicpRegister.cpp:42-45):
 * mean squared 1-NN distance of the last aligned source.  Negative when unavailable.
 * As in the reference the score is not part of scan2Map: the handle keeps a copy of the last aligned scan and its final pose, and
 * this call evaluates the score (once; later calls return the cached value) against the target the handle holds at that moment --
 * what PCL's getFitnessScore() does with input_, final_transformation_ and the current target tree.  1.797e308 (DBL_MAX) when no
 * point has a neighbour or no target is prepared, like PCL.  (A handle of a sharded target evaluates it with the alignment instead:
 * every rank takes part in the sum.)  The distances are PCL's float distances bit for bit; only the order of the double sum differs.
 * A voxel lattice that holds the scan's region only hands the search to the covariance search grid, which holds every point.  An index
 * cut to a region (a target too spread out for the dense tables: its bulk, or the room around a scan) answers only when every source point's
 * nearest indexed point is provably nearer than the cut faces; otherwise the score is taken on the sparse index of the kept target, which
 * holds every point (pcr_fitness_gated says how), and only where that index cannot be had this returns -1 and pcr_last_error names the cut
 * and the sparse index's reason.  pcr_params.query_index = PCR_QUERY_INDEX_SPARSE: always on the sparse index. */
double pcr_fitness(pcr_handle* h);

/* ---- introspection used by tests and bench.py ---- */

/* One LOAM linearisation at `pose` against the current target (pcr_set_target):
 * JtJ (36, row-major), JtE (6), accepted count.  Optional per-point outputs (host,
 * may be NULL): status[n] (0 accepted, 1 k-NN gate, 2 plane gate, 3 weight gate),
 * rows[n*7] (s*[n ; p x n], s*d), nn[n*5] (original target indices, ascending distance). */
int pcr_loam_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device,
                       const double pose[16], double JtJ[36], double JtE[6], int64_t* n_accepted,
                       int8_t* status, double* rows, int32_t* nn);

/* Per-iteration trace of the last LOAM call (params.record_trace = 1):
 * for it < *n_iters: JtJ[it*36..], JtE[it*6..], n[it], x[it*6..]. Arrays sized for loam_iters. */
int pcr_get_trace(pcr_handle* h, int32_t* n_iters, double* JtJ, double* JtE, int64_t* n, double* x);
/* Per linearisation of the last traced LOAM call: scan points whose neighbours came from the temporal
 * neighbour cache (proven exact) and points that needed a full grid search. */
int pcr_get_trace_counts(pcr_handle* h, int64_t* cache_hits, int64_t* searches);

/* VGICP introspection.  Per-point covariances as fast_gicp::FastGICP::calculate_covariances forms
 * them (fast_gicp_impl.hpp:241-297; 20-NN, PLANE regularisation): cov_out[n*6] = xx xy xz yy yz zz. */
int pcr_vgicp_covariances(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double* cov_out);
/* The neighbour lists behind the covariances of the LAST pcr_vgicp_covariances call on a scan-sized cloud (n <= 300 000):
 * nbr_out[n*20] = original indices of each point's 20 nearest neighbours (FLANN's float distances, ties on the lower index; the
 * point itself first), 0xffffffff where the cloud holds fewer; *queued_out = the queries the lane-per-query search handed to the
 * wave-per-query one (csrc/cov_search.hip).  fast_gicp_impl.hpp:250-253 (kdtree.nearestKSearch). */
int pcr_vgicp_neighbours(pcr_handle* h, size_t n, uint32_t* nbr_out, uint32_t* queued_out);
/* (pcr_vgicp_covariances and pcr_vgicp_neighbours serve gicp handles too: the covariances are the same.) */
/* One FastVGICP::linearize (fast_vgicp_impl.hpp:119-180) at `pose` against the current target
 * (pcr_set_target): H (36, row-major, twist = [rotation; translation]), b (6), sum of errors,
 * number of (source point, voxel) pairs -- under PCR_VGICP_DIRECT1 the source points with a voxel correspondence. */
int pcr_vgicp_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device,
                        const double pose[16], double H[36], double b[6], double* error, int64_t* n_corr);
/* GICP introspection (a gicp handle).  One FastGICP::update_correspondences + linearize (fast_gicp_impl.hpp:120-211) at `pose` against the kept
 * target (pcr_set_target): every source point transformed in float (a Matrix4f, as pcl::transformPointCloud), its nearest target point in
 * PCL's float metric (exact ties: the lower index), the gate d2 < (float)gicp_max_corr_dist^2, M = (C_B + R C_A R^T)^-1 in double; H (36,
 * row-major, twist = [rotation; translation]), b (6), *error = the sum of e^T M e, *n_corr = source points with a correspondence.
 * pose_eval (NULL, or a trial pose): *error_eval = compute_error(pose_eval) (:214-237) on the correspondences and matrices of the
 * linearisation at `pose`, nothing searched again (0 without pose_eval).  Optional per-point outputs (host, may be NULL): corr[n_src] = original
 * target index or -1, d2[n_src] = the correspondence's float squared distance (+inf where none), mahal6[n_src*6] = M as xx xy xz yy yz zz
 * (zeros where none). */
int pcr_gicp_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double pose[16],
                       const double* pose_eval, double H[36], double b[6], double* error, double* error_eval, int64_t* n_corr,
                       int32_t* corr, float* d2, double* mahal6);

/* ---- LIORF: LioScan2map of the reference's test/comp/liorf_scan2map.cpp (LIO-SAM's surface scan-to-map), a "liorf" handle ----
 * Everything is float.  The pose is six numbers, transformTobeMapped = [roll, pitch, yaw, x, y, z]; pcr_scan2map / pcr_align take the
 * six numbers out of the float cast of pose_inout once (pcr_liorf_pose_to_6dof), iterate on them on the device, and return
 * pcr_liorf_6dof_to_pose of the final six.  DESIGN.md ("liorf") has the definition operation by operation; in short, per iteration:
 * the float 4x4 of the six numbers; per scan point the float transform, the 5 nearest target points in PCL's float metric (ties on
 * the lower index), the gate d2[4] < liorf_knn_max_sq, the float 5x3 column-pivoted Householder QR plane fit, the residual gate, the
 * weight s and the row [arz, ary, arx, s pa, s pb, s pc | -s pd2] (the three angular entries are the exact derivatives of the residual:
 * one term of the file's line 310 is not, and is replaced unless liorf_file_row = 1); the 21 + 6 sums of the rows' products in double by the fixed-order
 * reduction, rounded to float once; the 6x6 system solved by Householder QR in float; the step ADDED to the six numbers.
 * *converged = the last iteration's step was below liorf_rot_conv_deg and liorf_trans_conv_cm.  pcr_stats.iterations = linearisations
 * performed: 0 when the scan has no more than liorf_min_scan points; a linearisation that keeps fewer than liorf_min_rows rows leaves
 * the pose alone and ends the call there (the file's loop would repeat that linearisation unchanged until its cap).
 * pcr_fitness() on a liorf handle is the file's own getFitnessScore: the mean of the float squared 1-NN distances d2 <= 1.0f of the
 * last aligned scan at the returned pose, -1 when there is none.  It runs on the machinery of pcr_fitness_gated, whose gate is the
 * same comparison -- a float distance, widened, against max_sq in double, '<=' -- so pcr_fitness_gated(max_sq = 1.0) is that score too.
 * pcr_relocalize / pcr_relocalize_global work on a liorf handle: their refinements are pcr_align. */

/* Host only (no GPU): pcl::getEulerAngles and the translation of a pose (16 doubles, column-major), through its float cast:
 * roll = atan2f(t21, t22), pitch = asinf(-t20), yaw = atan2f(t10, t00); out6 = [roll, pitch, yaw, x, y, z]. */
int pcr_liorf_pose_to_6dof(const double T[16], float out6[6]);
/* Host only: pcl::getTransformation(x, y, z, roll, pitch, yaw) = Rz(yaw) Ry(pitch) Rx(roll), formed in float from A = cosf(yaw),
 * B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll):  row 0 = [A C, A D F - B E, B F + A D E, x],
 * row 1 = [B C, A E + B D F, B D E - A F, y], row 2 = [-D, C F, C E, z]; widened to 16 doubles, column-major. */
int pcr_liorf_6dof_to_pose(const float in6[6], double T[16]);
/* One linearisation (surfOptimization + the sums of LMOptimization) at the six numbers `six` against the kept target (pcr_set_target).
 * T_used: the float 4x4 the DEVICE built from them, row-major (a reference can run the per-point stage on exactly that matrix).
 * Per point (host arrays, may be NULL): kept[n] = 1 when the point gave a row; coeff4[n*4] = (s pa, s pb, s pc, s pd2), zeros where
 * not kept.  AtA (36, row-major) and AtB (6): the double sums before the rounding to float; *n_kept = the rows. */
int pcr_liorf_linearize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const float six[6],
                        float T_used[16], uint8_t* kept, float* coeff4, double AtA[36], double AtB[6], int64_t* n_kept);
/* The last pcr_scan2map / pcr_align of a liorf handle: the final six numbers, isDegenerate (iteration 0: the smallest eigenvalue of the
 * float AtA is below liorf_degenerate_eig; 0 when iteration 0 solved nothing) and the rows kept by the last linearisation. */
int pcr_liorf_result(pcr_handle* h, float six[6], int* degenerate, int64_t* rows_last);

/* pcl::VoxelGrid<PointXYZI>::filter (leaf, leaf, leaf) -- the step before the path: every scan at
 * frontend/src/LidarOdometry.cpp:36,170-171, every rebuilt sub-map at frontend/src/MapManager.cpp:78,192 through
 * common/pcp/pcp.hpp:14-28.  One centroid per occupied voxel of PCL's lattice (idx = floor(p / leaf) - min_b, float
 * arithmetic as in PCL), all fields averaged, output in ascending voxel index.  Points keep the input stride; with the
 * 32-byte pcl::PointXYZI layout data[3] = 1 and the intensity (float 4) is averaged, with a 16-byte layout float 3 is.
 * Non-finite points are skipped.  *n_out = number of voxels (also when out_capacity was too small, so that the caller
 * can retry).  A leaf so small that PCL's integer voxel index would overflow returns the input unfiltered, like PCL.
 * Works on any handle (the method is irrelevant). */
int pcr_voxel_filter(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double leaf, void* out,
                     size_t out_capacity, int out_on_device, size_t* n_out);

/* The same in two halves, device memory in and out: _begin queues the filter on the handle's stream and returns, _end waits for it and returns the voxel
 * count (the filter's one synchronisation).  For a caller that has the NEXT scan while this one is being registered -- replaying a recording, or a
 * front end that lags its sensor: filter it on a second handle (a stream of its own) meanwhile.  out_capacity >= n; input and output stay untouched until _end.
 * One filter per handle at a time (pcr_voxel_filter on that handle in between is refused). */
int pcr_voxel_filter_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity);
int pcr_voxel_filter_end(pcr_handle* h, size_t* n_out);

/* ---- A scan's motion distortion undone (deskew): every point moved into the sensor frame of ONE time of the sweep ------------------------
 * The reference never does this (pcl::PointXYZI has no time field); a spinning lidar collects a sweep over ~0.1 s, and at 2 m/s and 0.5 rad/s
 * its last point is displaced by 20 cm and 0.05 rad from its first.  The caller supplies the sensor's MOTION, the library applies it per point.
 *   Motion: K control poses (2 <= K <= 1024; pose j = poses[16 j ..], the layout of every pose[16] here, the sensor's pose in any one fixed
 *   frame) at strictly increasing finite stamps[K] (seconds).  A point's time is tau = t0 + its time field, by time_kind below.
 *   Definition (csrc/deskew_math.h, f64 + - * / sqrt alone, every operation rounded on its own, so host and device give the same bits):
 *   each rotation goes to a unit quaternion by Eigen's Quaternion(Matrix3) (the trace branch, else the largest diagonal element), negated
 *   where its four-term dot product with its predecessor's is negative.  At a time tau, clamped to [stamps[0], stamps[K-1]], j is the largest
 *   index of [0, K-2] with stamps[j] <= tau, s = (tau - stamps[j]) / (stamps[j+1] - stamps[j]), u = 1.0 - s, every component of the
 *   quaternion and of the translation is u*a + s*b, the quaternion is divided by n = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3) and becomes a
 *   rotation matrix R by Eigen's toRotationMatrix.  That is normalised linear interpolation: its rotation differs from one of constant
 *   angular velocity by at most theta^3 / 240 rad in a segment that turns by theta <= 1 rad (5.7e-7 rad at 3 degrees, 2.1e-5 rad at 10): a
 *   caller who wants less supplies denser control poses.  A point (x, y, z) widened to double becomes y_r = ((R_r0 x + R_r1 y) + R_r2 z) +
 *   p_r at its own time and z = R_ref^T (y - p_ref), summed in the same association, at t_ref; z rounded to float replaces the coordinates and
 *   every other byte of the record is copied.  (An all-identity motion returns the input bit for bit, a coordinate of -0 as +0.)
 *   A record with a non-finite coordinate or a non-finite tau is copied unchanged and counted in info->nonfinite.
 *   Time source: times != NULL is a packed array of n elements of the kind, living where pts lives; times == NULL reads a field of every
 *   record at time_offset_bytes (Velodyne's 32-byte PointXYZIRT: PCR_TIME_F32_SECONDS at byte 24), which must be a multiple of the
 *   element's size, not below 12 and with the whole field inside stride_bytes.
 *   Output: n records of the input's stride_bytes (>= 16, a multiple of 4).  out == pts (in place) is allowed; any other overlap of out with
 *   pts or times inside one memory space is refused.  info (may be NULL): the points whose time was clamped at either end, the records copied
 *   unchanged, and whether t_ref was clamped.  n == 0 succeeds and writes nothing but *info.
 *   Refused with a message that names the field, before anything is written: K outside 2..1024; stamps not strictly increasing or not finite;
 *   poses, t0 or t_ref not finite, or a pose whose rotation yields no finite unit quaternion; an unknown time_kind; a bad
 *   time_offset_bytes or stride_bytes; NULL pts, out, m, m->poses or m->stamps.
 * pcr_deskew_host is the definition: host memory, no GPU; pcr_last_error(NULL) holds its refusal.  pcr_deskew is the same on the device, one
 * launch on the handle's stream (any method; pcr_last_error(h)), pts / times and out each in host or device memory: a raw scan uploaded once
 * can stay in HBM from here through the filter, the registration and the key-frame store.  The two agree bit for bit. */
#define PCR_TIME_F32_SECONDS 0      /* tau = t0 + (double)f            */
#define PCR_TIME_U32_NANOSECONDS 1  /* tau = t0 + (double)u * 1e-9     */
#define PCR_TIME_F64_SECONDS 2      /* tau = t0 + d                    */
typedef struct pcr_deskew_motion { const double* poses; const double* stamps; size_t K; double t0; double t_ref; } pcr_deskew_motion;
typedef struct pcr_deskew_info { int64_t before, after, nonfinite; int32_t ref_clamped; } pcr_deskew_info;
int pcr_deskew(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, const void* times, int time_kind,
               long long time_offset_bytes, const pcr_deskew_motion* m, void* out, int out_on_device, pcr_deskew_info* info);
int pcr_deskew_host(const void* pts, size_t n, size_t stride_bytes, const void* times, int time_kind, long long time_offset_bytes,
                    const pcr_deskew_motion* m, void* out, pcr_deskew_info* info);

/* ---- the reference's own sparse voxel filters: pcp::VoxelDownSampleV3 and pcp::VoxelDownSampleV2 (common/pcp/pcp.hpp:157-263, :78-154) ----
 * pcl::VoxelGrid -- and pcr_voxel_filter with it -- gives up once the voxel box exceeds INT_MAX cells.  These two hold the occupied voxels
 * only: device memory grows with n, never with the box.  Same argument conventions as pcr_voxel_filter: any handle, records of stride_bytes
 * with x, y, z as floats first, the output record's fields by the rule of the 16- and 32-byte layouts, *n_out = the voxel count also when
 * out_capacity was too small (the call then fails and the caller can retry), leaf cast to float (the reference's `float gs`).
 *   Both kinds.  A row with a non-finite coordinate is dropped and renumbers nothing (the reference casts such a value to an integer, which
 *   is undefined).  An empty input, or one without a finite row, gives *n_out = 0 and rc 0.  A voxel is its integer triple; the kept rows'
 *   triples, each axis relative to its smallest value over the kept rows, are packed into one 64-bit key -- z most significant, then y, then
 *   x, an axis of extent e taking bits(e - 1) bits -- and the (key, row) pairs are sorted by a stable radix sort.  OUTPUT ORDER: ascending
 *   key, i.e. ascending (z, y, x) -- pcr_voxel_filter's order, so the two compare row for row where both filter.  (The reference's own order
 *   is std::unordered_map's and specifies nothing.)  The same call twice gives the same bytes.
 *   Refused, with a message: a cloud whose three extents need more than 64 key bits (the message gives the extents; the reference's size_t
 *   index wraps), a cloud in which floor(p * inv) (V3) or p / gs (V2) leaves the int range on a kept row (undefined in the reference),
 *   a non-positive leaf, max_voxel_pts < 1, min_voxel_pts < 0, an unknown kind -- each named.
 *   V3 (pcp.hpp:172-254): inv = 1.0f / gs, min_b = (int)floor(min_p * inv), ijk = floor(p * inv) - (float)min_b, all in float without
 *   contraction: pcl::VoxelGrid's lattice without its too-fine test.  Output: the centroid of all fields (pcl::CentroidPoint), data[3] = 1 in
 *   the 32-byte layout; sums in double in sorted order, rounded to float once.
 *   V2 (pcp.hpp:102-152, KISS-ICP's voxel hash): voxel = (int)(p / gs), a float division truncated toward zero -- the voxels touching zero
 *   are two leaves wide on that axis.  Per voxel the max_voxel_pts rows of lowest index are kept; the voxel is emitted when that count is
 *   strictly greater than min_voxel_pts; the record is the lowest-index row's bytes with x, y, z replaced by the float mean: a sequential
 *   float sum in ascending row index divided by (float)count. */
#define PCR_VOXEL_SPARSE_V3 3     /* pcp::VoxelDownSampleV3, pcp.hpp:157-263 */
#define PCR_VOXEL_SPARSE_V2 2     /* pcp::VoxelDownSampleV2, pcp.hpp:78-154  */
typedef struct {
    int32_t kind;              /* default V3 */
    int32_t max_voxel_pts;     /* V2 only, default 20 */
    int32_t min_voxel_pts;     /* V2 only, default 0  */
} pcr_voxel_sparse_params;
void pcr_voxel_sparse_default_params(pcr_voxel_sparse_params* p);
/* p = NULL: the defaults */
int  pcr_voxel_filter_sparse(pcr_handle* h, const void* pts, size_t n, size_t stride_bytes, int on_device, double leaf,
                             const pcr_voxel_sparse_params* p, void* out, size_t out_capacity, int out_on_device, size_t* n_out);
/* what the last sparse call on this handle sorted: per kept input row, in sorted order, its packed voxel key and its original row index.
 * *count = the kept rows (also when capacity was too small: the call then fails and writes nothing else); keys / rows may be NULL.  Fails
 * when the handle's last sparse call was refused or none was made. */
int  pcr_voxel_sparse_order(pcr_handle* h, uint64_t* keys, uint32_t* rows, size_t capacity, size_t* count);

/* ---- the producer of `dst`: MapManager's key-frame store and sub-map assembly, on the device ----
 * MapManager::updateMap (frontend/src/MapManager.cpp:151-201): key frames whose position lies within `radius`
 * (mSurroundingKeyframeSearchRadius = 8 m, MapManager.hpp:68; squared L2 in double, strict '<' like
 * KeyFramesKdtree::radiusSearch, kfs_adaptor.hpp:57-75) are transformed by their pose cast to float
 * (pcp::transformPointCloud, common/pcp/pcp.hpp:38-62), concatenated and voxel-filtered with grid_size
 * (pcp::voxelDownSample, pcp.hpp:14-20).  Key frames are copied into HBM when added; the assembled sub-map stays in
 * HBM and is handed to pcr_scan2map_device / pcr_set_target as `dst` (pcr_map_submap: pointer valid until the next
 * pcr_map_update or pcr_map_destroy).  pcr_map_submap_indices = mSubmapIdx (ascending key-frame index). */
typedef struct pcr_map pcr_map;
pcr_map* pcr_map_create(int device);                    /* device ordinal, -1 = current; NULL on failure (pcr_map_last_error(NULL)) */
void pcr_map_destroy(pcr_map* m);
const char* pcr_map_last_error(const pcr_map* m);
/* KeyFrame{pc, pose} (common/types/basic.hpp:33-40); pose = 16 doubles column-major.  Index of the new key frame = count - 1. */
int pcr_map_add_keyframe(pcr_map* m, const void* pts, size_t n, size_t stride_bytes, int on_device, const double pose[16]);
int pcr_map_keyframes(const pcr_map* m, size_t* n_keyframes);
/* Forget every key frame and the sub-map (a new session: MapManager::reset), keep the device memory the store has grown to; starts a new generation. */
int pcr_map_clear(pcr_map* m);
int pcr_map_update(pcr_map* m, const double position[3], double radius, double grid_size, size_t* n_submap);
/* The same in two halves, for a caller that has something else to do meanwhile -- the reference assembles its sub-map on a map thread of its own
 * (frontend/src/MapManager.cpp:109-119 notifies it and LidarOdometry goes on with the next scan): pcr_map_update_begin selects the key frames, starts a
 * new generation and QUEUES the assembly on the map's stream; pcr_map_wait collects it (the update's one synchronisation; errors of the assembly are
 * reported here).  Every call that needs the sub-map (pcr_map_submap, pcr_scan2map_submap) or changes the store (pcr_map_add_keyframe, another update)
 * collects a queued assembly first, so the result never depends on when the wait happens: pcr_map_update = begin + wait.
 * (A pcr_map, like a pcr_handle, is used by one thread at a time: the overlap is between the device's streams, not between host threads.) */
int pcr_map_update_begin(pcr_map* m, const double position[3], double radius, double grid_size);
int pcr_map_wait(pcr_map* m, size_t* n_submap);
/* LoopClosureManager::loopFindNearKeyframes (backend/src/LoopClosureManager.cpp:40-60): key frames key - search_num .. key + search_num
 * (clipped to the store), transformed, concatenated, voxel-filtered: the target of the loop-closure registration (:96-99). */
int pcr_map_update_window(pcr_map* m, long long key, int search_num, double grid_size, size_t* n_submap);
const void* pcr_map_submap(const pcr_map* m, size_t* n, size_t* stride_bytes);
int pcr_map_submap_indices(const pcr_map* m, int64_t* idx, size_t capacity, size_t* n);
/* ---- the store's life beyond the front end: what the back end does to MapManager's key frames ----
 * Backend::optimHandler (backend/src/Backend.cpp:315-318): replace the poses of key frames first .. first+count-1 (16 doubles each,
 * column-major).  Fails, leaving the store as it was, when first + count exceeds the key-frame count, when poses is NULL with count > 0, and
 * on a view; count == 0 is a no-op.  No assembled sub-map (the parent's or a view's), no selection and no generation is touched -- the
 * reference's mSubmap is left alone until the next updateMap too; the next pcr_map_update* on the parent or on a view selects by the new
 * translations and transforms by the new poses cast to float.  An assembly that is queued (pcr_map_update_begin, on the parent or on a view)
 * was selected under the old poses and finishes as such: it is waited for first. */
int pcr_map_set_poses(pcr_map* m, size_t first, size_t count, const double* poses);
/* Key frame i as it is stored (parent or view): device pointer -- valid until the next call that changes the store -- point count, stride and
 * pose; the bytes are exactly those stored, stride_bytes / 4 floats per point.  NULL with pcr_map_last_error for an index out of range; NULL
 * with *n = 0 for a key frame of 0 points.  This is lc_scan_ of LoopClosureManager::lcHandler (LoopClosureManager.cpp:92) without a host copy. */
const void* pcr_map_keyframe(const pcr_map* m, size_t i, size_t* n, size_t* stride_bytes, double pose[16]);
/* The same to host memory.  *n is always the key frame's size; when capacity_points < *n the call fails and writes nothing else. */
int pcr_map_read_keyframe(const pcr_map* m, size_t i, void* out, size_t capacity_points, size_t* n, double pose[16]);
/* MapManager::saveKfs (frontend/src/MapManager.cpp:211) and the loading constructor (:46): every key frame i >= first, in ascending order,
 * is replaced by what pcr_voxel_filter gives for its cloud at grid_size, byte for byte (ascending voxel index; a grid too fine for PCL's
 * integer voxel index leaves the key frame unchanged).  Key frames before `first` keep their offsets and bytes, the later ones are packed
 * directly behind them and the store shrinks; its device memory is kept.  *store_points_after = points in the store afterwards.
 * first == count is a no-op; first > count, a non-positive grid_size and a call on a view are errors.  Sub-maps already assembled, their
 * selections and generations are untouched; queued assemblies on the parent and on all views are waited for first (they read the store).
 * Should a filter fail, the key frames in front of the failing one stay filtered and every key frame stays readable. */
int pcr_map_downsample_keyframes(pcr_map* m, size_t first, double grid_size, size_t* store_points_after);
/* The session's product (test/vis_globalmap.cpp:33-66, and the file MapManager(pcd_file) loads): EVERY key frame selected, otherwise exactly
 * pcr_map_update -- a new generation, transform, concatenate, voxel-filter; more than 0xfffffff0 points are an error, and a map whose extent
 * is beyond pcl::VoxelGrid's index range at grid_size comes back unfiltered, as PCL returns it.  Parent or view. */
int pcr_map_update_all(pcr_map* m, double grid_size, size_t* n_submap);
/* pcr_map_update_all with pcp::VoxelDownSampleV3 in place of pcl::VoxelGrid: every key frame selected, a new generation, the same transform
 * pass and 0xfffffff0 cap, a queued assembly collected first; the sub-map is byte for byte pcr_voxel_filter_sparse (V3) of the concatenation,
 * so a map of any extent comes back filtered (more than 64 key bits are an error).  Parent or view. */
int pcr_map_update_all_sparse(pcr_map* m, double grid_size, size_t* n_submap);
/* A second (third, ...) sub-map over the SAME key frames: LoopClosureManager's lc_map_ (LoopClosureManager.cpp:85-99) beside MapManager's
 * mSubmap.  The view has its own stream and filter, concatenation, sub-map, selection, queued-assembly state, id and generation, on the
 * parent's device; it reads the parent's key frames, poses and point layout.  NULL on failure (pcr_map_last_error(parent)).
 *   On a view work: pcr_map_update, _update_begin, _wait, _update_window, _update_all, _submap, _submap_indices, _generation, _keyframes,
 *   _keyframe, _read_keyframe, pcr_scan2map_submap, pcr_map_destroy.
 *   On a view fail, with a message that says it is a view: pcr_map_add_keyframe, _clear, _set_poses, _downsample_keyframes, pcr_map_view.
 * The parent waits for every view's queued assembly before the store moves (pcr_map_add_keyframe), shrinks (_downsample_keyframes) or is
 * emptied (_clear); pcr_map_clear also empties every view's selection and sub-map and starts a new generation on each.
 * pcr_map_destroy(parent) waits for its views and detaches them: a detached view fails every call with "parent destroyed", except
 * pcr_map_destroy(view), which frees it.  pcr_map_destroy(view) unregisters it from a living parent.
 * THREADS (the reference's mLockKF: LoopClosureManager.cpp:27,39,89, MapManager.cpp:175): a view may be driven by another thread than its
 * parent.  Calls that change the store -- pcr_map_add_keyframe, _clear, _set_poses, _downsample_keyframes and pcr_map_destroy of the parent
 * -- must not overlap with ANY call on a view of it: that is the caller's lock.  Sub-map calls on the parent and on its views (_update*,
 * _wait, _submap, pcr_scan2map_submap) may overlap with each other; each single pcr_map is still used by one thread at a time. */
pcr_map* pcr_map_view(pcr_map* parent);
/* Identity of the store and of the sub-map it currently holds: every pcr_map_update / pcr_map_update_window starts a new
 * generation.  This is the explicit version of what the reference's registrars approximate by comparing cloud POINTERS
 * (fast_gicp_impl.hpp:83-90): a structure built for generation g is valid exactly while the map reports g. */
int pcr_map_generation(const pcr_map* m, uint64_t* id, uint64_t* generation);
/* scan2Map against the sub-map `m` currently holds (stride = the map's).  The handle keeps the target structures it builds
 * -- LOAM's grid index, NDT's voxel Gaussians, VGICP's covariances and voxel map -- together with (id, generation) of the
 * sub-map they were built from and rebuilds them only when the map has moved on: LidarOdometry registers several scans
 * against one sub-map between two MapManager updates (frontend/src/LidarOdometry.cpp:184, MapManager.cpp:151-201).  Same
 * result as pcr_scan2map_device on pcr_map_submap(m), bit for bit. */
int pcr_scan2map_submap(pcr_handle* h, const void* src, size_t n_src, int src_on_device, const pcr_map* m,
                        double pose_inout[16], int* converged);

/* ---- the loop-closure descriptor: backend/src/ScanContext.cpp (20 rings x 60 sectors over 80 m) ----
 * pcr_sc_add = addContext (:56-66): the polar binning of the (down-sampled, lidar-frame) scan runs on the device, the ring
 * and sector keys follow on the host.  pcr_sc_query = query (:231-279): the 10 nearest ring keys among the contexts
 * older than num_exclude_recent (a snapshot refreshed every build_tree_gap contexts, as the reference's lazily rebuilt
 * tree), each compared by distanceBtnScanContext (:116-150); *match = -1 when the best distance exceeds dist_thres. */
typedef struct pcr_sc pcr_sc;
typedef struct pcr_sc_params {
    double lidar_height;          /* 2.0  config/params.json tf.lidar_height */
    int32_t num_exclude_recent;   /* 40   backend.context.scancontext.numExcludeRecent */
    int32_t build_tree_gap;       /* 10 */
    int32_t num_candidates;       /* 10   numCandidatesFromTree */
    int32_t pad;
    double search_ratio;          /* 0.1 */
    double dist_thres;            /* 0.4  scDistThres */
} pcr_sc_params;
void pcr_sc_default_params(pcr_sc_params* p);
pcr_sc* pcr_sc_create(int device, const pcr_sc_params* p);
void pcr_sc_destroy(pcr_sc* sc);
const char* pcr_sc_last_error(const pcr_sc* sc);
int pcr_sc_size(const pcr_sc* sc, size_t* n);
int pcr_sc_add(pcr_sc* sc, const void* pts, size_t n, size_t stride_bytes, int on_device);
/* LoopClosureManager::addContext (backend/src/LoopClosureManager.cpp:28-37) over key frames [first, first + count) of a key-frame store, parent or
 * view, in one batched pass: one context per key frame, in key-frame order, from the key frame's stored points in the lidar frame as
 * pcr_map_keyframe returns them (its pose is not applied).  Every new context -- the row of the device store and the host's descriptor, ring key
 * and sector key -- is bit for bit what pcr_map_keyframe -> pcr_voxel_filter at leaf grid_size -> pcr_sc_add of the filter's output leaves, so
 * every reader (pcr_sc_descriptor, _distance, _query, _distances, _rank_stored, pcr_relocalize_global) works on it unchanged.  grid_size <= 0: no
 * filter, the stored points are binned as they are (key frames already filtered by pcr_map_downsample_keyframes: a loaded map); the whole range is
 * then one table up, one launch and one copy back, with no synchronisation per key frame.  grid_size > 0: the key frames pass the voxel filter one
 * by one, on a handle the database creates at the first such call, into one packed buffer (room for the unfiltered points of the range), which is
 * binned the same way; a key frame the filter returns unfiltered (a grid too fine for PCL's voxel index) is binned as returned.  A key frame of 0
 * points adds an all-empty context, as pcr_sc_add with n = 0 does.  count == 0 succeeds and adds nothing; *n_added (may be NULL) = count.
 * The device store grows straight to the capacity its doubling rule reaches for the new size: one allocation and one copy.
 * Fails with a message in pcr_sc_last_error, the database left as it was (size, stored contexts, host entries), when sc or m is NULL (sc NULL:
 * pcr_sc_last_error(NULL)), first + count exceeds pcr_map_keyframes(m), m is a view whose parent was destroyed, sc and m are on different devices,
 * the store cannot grow, or on any HIP or filter error.  m is used as pcr_map_keyframe uses it: no call that changes the store may overlap. */
int pcr_sc_add_keyframes(pcr_sc* sc, const pcr_map* m, size_t first, size_t count, double grid_size, size_t* n_added);
int pcr_sc_descriptor(const pcr_sc* sc, size_t id, double* desc_row_major_20x60, double* ring_key_20, double* sector_key_60);
int pcr_sc_distance(const pcr_sc* sc, size_t id1, size_t id2, double* dist, int* shift);
int pcr_sc_query(pcr_sc* sc, long long id, long long* match, float* yaw_rad, double* min_dist);
/* distanceBtnScanContext of an outside scan (lidar frame, not added) against EVERY stored context, on the device.
 * dist[i], shift[i] are exactly what pcr_sc_distance(q, i) returns if the same cloud were added as context q:
 * same sector-key alignment, same 2*round(0.5*(float)search_ratio*60)+1 shifts in ascending order, strict '<',
 * DBL_MAX / 0 for a context against which every column is empty. dist, shift: pcr_sc_size() entries each.
 * Every context's descriptor is kept in HBM as float (4 800 B each, what pcr_sc_add binned); the query is binned into a scratch
 * buffer and never enters the database.  On an empty database the call returns 0 and writes nothing. */
int pcr_sc_distances(pcr_sc* sc, const void* pts, size_t n, size_t stride_bytes, int on_device, double* dist, int32_t* shift);
/* Loop discovery over a range of STORED contexts, on the device: for every query q of [first, first + count) and every candidate i of
 * [0, q - num_exclude_recent), (dist, shift) exactly as pcr_sc_distance(sc, q, i) returns them (the query unshifted, the candidate
 * shifted: the function is not symmetric), and of those the k best by (dist, i) ascending -- the lower index wins a tie.  Row q - first
 * of idx, dist, shift (count * k entries each) holds them in that order; where q has fewer than k candidates (none at all while
 * q <= num_exclude_recent) the tail is idx -1, dist DBL_MAX, shift 0.  A candidate at DBL_MAX (no non-empty column pair under any shift)
 * is a candidate like any other and so sorts last, by index.  dist_thres is not applied: this is the ranking (the mirrors' findLoops
 * applies it).  The reference's query refuses id <= numExcludeRecent + numCandidatesFromTree because its ring-key tree needs 10 entries to
 * answer; the exhaustive ranking has no such floor, and it is never worse than the tree's 10 candidates.  k is 1..8.
 * Fails with a message in pcr_sc_last_error, writing NOTHING, when k is out of range, first + count > pcr_sc_size(), or idx, dist or
 * shift is NULL while count > 0; count == 0 returns 0.  The same call gives the same bits whatever the window: a row depends on its
 * query alone.  The database and the candidate snapshot of pcr_sc_query are left as they are (the call caches each context's column
 * norms and sector key in HBM, 960 B per context, computed once). */
int pcr_sc_rank_stored(pcr_sc* sc, size_t first, size_t count, int k, int64_t* idx, double* dist, int32_t* shift);
/* Host-only: the yaw of a match, trans::deg2rad<float>(6 degrees * shift), as pcr_sc_query forms it. */
float pcr_sc_shift_yaw(int32_t shift);

/* ---- the pose-graph back end: Backend::optimHandler (backend/src/Backend.cpp:224-347), on the device ----
 * An SE(3) pose graph of prior and between factors, optimised by Levenberg-Marquardt whose linear solve is a preconditioned conjugate
 * gradient that runs wholly on the device.  GTSAM is not reproduced bit for bit; the contract is this definition:
 *   poses     16 doubles, column-major, like every pose of this header.  Tangent vectors are [omega; v], rotation first (GTSAM's Pose3 order);
 *             the update is X <- X Exp(delta) with the full SE(3) exponential.
 *   between   (from, to, Z, Omega): r = Log(Z^-1 X_from^-1 X_to).        prior (id, P, Omega): r = Log(P^-1 X_id).
 *   Omega     a full symmetric 6x6 information matrix in [omega; v] order, passed as its 21 upper-triangular entries, row by row.
 *   cost      1/2 sum r^T Omega r;  chi2 = sum r^T Omega r.  Jacobians are exact (the inverse right Jacobian of SE(3)).
 *   optimiser (H + lambda I) delta = -g, H = sum J^T Omega J.  A step is accepted when chi2 falls; lambda is divided by lambda_factor on
 *             acceptance and multiplied on rejection.  It stops when an accepted step lowered chi2 by less than abs_tol or by less than
 *             rel_tol * chi2 (converged), when a rejected step raised chi2 by less than abs_tol (converged), when lambda exceeds
 *             lambda_max, or after max_iterations trial steps.
 *   robust    a between factor that carries the robust mark (pcr_graph_add_loop, pcr_graph_set_between_robust) enters through the graph's
 *             kernel (pcr_graph_set_robust_kernel): with s = r^T Omega r it adds rho(s) to chi2, w(s) J^T Omega r to g and w(s) J^T Omega J
 *             to H, w = rho' (the second-order term is dropped, as g2o and GTSAM drop it).  The cost is 1/2 sum rho; the optimiser accepts
 *             and stops on sum rho.  Priors and unmarked between factors are never robust.  A between factor that is switched off
 *             (pcr_graph_set_between_enabled) adds nothing to chi2, g and H and links nothing.  Under the defaults -- kernel NONE, every
 *             factor on -- everything above is as if this paragraph were absent, bit for bit.
 *   fixed     a pose that carries the fixed flag (pcr_graph_set_fixed, a FIX record of a g2o file) is a constant of the problem: the unknowns
 *             are the free poses, the normal equations those of the full problem without the fixed poses' rows and columns, and every
 *             pcr_graph_optimize leaves a fixed pose's 16 doubles as they were, bit for bit.  chi2 stays the sum over every factor that is on
 *             (one between two fixed poses is a constant term; it counts), robust weights are as above.  A fixed pose anchors its connected
 *             component as a prior does.  With no flag set everything is as if this paragraph were absent, bit for bit.
 * Ids are positions: the poses are numbered from 0 in the order they were added.  Factors may be added before their poses; the graph is
 * checked when it is used.  A pcr_graph is used by one thread at a time. */
typedef struct pcr_graph pcr_graph;
#define PCR_GRAPH_HOST (-2)
enum { PCR_GRAPH_PRIOR = 0, PCR_GRAPH_ODOM = 1, PCR_GRAPH_LOOP = 2 };
/* The preconditioner M of the conjugate gradient.
 *   BLOCK_JACOBI  every pose's 6x6 diagonal block of H + lambda I.  Information moves one edge per iteration: right for the tens to hundreds
 *                 of key frames one event meets, and for graphs dense in loop edges (a hub with full information matrices).
 *   TREE          lambda I + every prior + the between factors of a spanning forest, solved exactly by a block Cholesky without fill (two
 *                 sweeps over the poses per iteration).  The forest: the between factors in the order added, each joining when its ends lie in
 *                 different components -- Backend::addOdomFactor's edges, one per key frame, are that forest; every other between factor is
 *                 left to the conjugate gradient.  Right for an odometry tree plus few loops at thousands of poses (a loaded map); on a hub
 *                 graph with many loops it can need MORE iterations than BLOCK_JACOBI. */
enum { PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1 };
typedef struct pcr_graph_params {
    uint32_t struct_size;          /* sizeof(pcr_graph_params), set by pcr_graph_default_params */
    int32_t max_iterations;        /* 100: trial steps (GTSAM's LevenbergMarquardtParams defaults throughout) */
    double rel_tol, abs_tol;       /* 1e-5, 1e-5 */
    double lambda_init, lambda_factor, lambda_max;      /* 1e-5, 10, 1e5 */
    int64_t pcg_max_iterations;    /* 0 = max(100, 10 * poses) */
    double pcg_rel_tol;            /* 1e-10, on |residual| / |g| */
    int32_t pcg_preconditioner;    /* PCR_GRAPH_PRECOND_BLOCK_JACOBI; another value than the two above is refused */
} pcr_graph_params;
typedef struct pcr_graph_result {
    int32_t iterations, accepted;  /* trial steps (one linear solve each); those that were accepted */
    int64_t pcg_iterations;        /* over all solves */
    int32_t pcg_capped;            /* solves that pcg_max_iterations ended */
    int32_t converged;
    double chi2_initial, chi2_final, lambda;
    double delta[16];              /* X_last after * X_last before ^-1 for the highest id, re-orthonormalised as trans::T2SE3 does: what optimHandler
                                      hands to the front end (Backend.cpp:321-346); the identity when that pose is fixed */
} pcr_graph_result;
/* device: an ordinal, -1 = current, PCR_GRAPH_HOST = no device at all (everything but optimize and apply works; linearize runs on the host
 * through the same header the kernels compile).  NULL on failure (pcr_graph_last_error(NULL)). */
pcr_graph* pcr_graph_create(int device);
void pcr_graph_destroy(pcr_graph* g);
const char* pcr_graph_last_error(const pcr_graph* g);
/* The reference's three diagonal noise models (Backend.cpp:90-97; variances, so Omega = diag(1 / variance)):
 * PRIOR 1e-2 1e-2 pi/72 1e-1 1e-1 1e-1, ODOM 1e-4 x3 1e-1 x3, LOOP 1e-1 x6.  Nonzero for another kind. */
int pcr_graph_noise(int kind, double info21[21]);
int pcr_graph_add_poses(pcr_graph* g, const double* poses16, size_t count);         /* ids are consecutive from 0 */
int pcr_graph_add_prior(pcr_graph* g, size_t id, const double pose[16], const double info21[21]);
int pcr_graph_add_between(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]);
/* z = X_from^-1 X_to of the current estimates (Backend::addOdomFactor, Backend.cpp:241-247); both ids must exist */
int pcr_graph_add_between_poses(pcr_graph* g, size_t from, size_t to, const double info21[21]);
/* Robust kernels on s = r^T Omega r, d = delta^2 (the square of a residual's Mahalanobis length where the kernel departs from least squares):
 *   NONE           rho = s                                                   w = 1
 *   HUBER          rho = s (s <= d), 2 delta sqrt(s) - d beyond              w = 1, delta / sqrt(s)
 *   GEMAN_MCCLURE  rho = d s / (d + s)                                       w = d^2 / (d + s)^2
 *   TUKEY          rho = d/3 (1 - (1 - s/d)^3) (s <= d), d/3 beyond          w = (1 - s/d)^2, 0
 * Cauchy is absent on purpose: its rho needs a logarithm, and this back end calls no math library (that is how host and device agree bit
 * for bit); these need + - * / sqrt only.  GEMAN_MCCLURE and TUKEY redescend: the optimum they reach depends on the start.  TUKEY reaches
 * w = 0, so marking odometry edges can leave H singular but for lambda I -- the caller's choice, not refused. */
enum { PCR_GRAPH_ROBUST_NONE = 0, PCR_GRAPH_ROBUST_HUBER = 1, PCR_GRAPH_ROBUST_GEMAN_MCCLURE = 2, PCR_GRAPH_ROBUST_TUKEY = 3 };
/* The graph's kernel for its marked between factors (NONE until set; pcr_graph_clear keeps it).  Another kind is refused; delta must be finite
 * and greater than 0 unless kind is NONE. */
int pcr_graph_set_robust_kernel(pcr_graph* g, int kind, double delta);
int pcr_graph_get_robust_kernel(const pcr_graph* g, int* kind, double* delta);
/* Marks (on != 0) or unmarks between factors first .. first+count-1, by index among the between factors in the order added. */
int pcr_graph_set_between_robust(pcr_graph* g, size_t first, size_t count, int on);
/* Switches between factors on or off, same indexing.  One that is off is left out of chi2, g and H, of the connectivity check (a component
 * that loses its only link to a prior is refused, its first pose named) and of PCR_GRAPH_PRECOND_TREE's forest and pcr_graph_tree's counts.
 * It stays in pcr_graph_size, in pcr_graph_linearize's r and J and in pcr_graph_save_g2o.  Setting the kernel, a mark or a switch counts as
 * something new for pcr_graph_optimize. */
int pcr_graph_set_between_enabled(pcr_graph* g, size_t first, size_t count, int on);
/* Fixes (on != 0) or frees poses first .. first+count-1.  A range beyond the poses is refused and changes nothing.  Setting or clearing a flag
 * counts as something new for pcr_graph_optimize; pcr_graph_clear drops the flags with the poses.  pcr_graph_fixed reads them back, one byte
 * per pose (1: fixed). */
int pcr_graph_set_fixed(pcr_graph* g, size_t first, size_t count, int on);
int pcr_graph_fixed(const pcr_graph* g, size_t first, size_t count, uint8_t* fixed);
/* pcr_graph_add_between plus the robust mark (under NONE the mark changes nothing) */
int pcr_graph_add_loop(pcr_graph* g, size_t from, size_t to, const double z[16], const double info21[21]);
/* The verdict, at the current estimates, on device and host graphs (bit for bit alike): for between factors first .. first+count-1, s = r^T Omega r
 * and the weight w the graph's kernel gives at s (1 for an unmarked factor; for one that is off, the weight it would have if switched on),
 * the mark and the switch.  Any output pointer may be NULL. */
int pcr_graph_between_weights(pcr_graph* g, size_t first, size_t count, double* s, double* w, uint8_t* robust, uint8_t* enabled);
/* Host only: rho(s) and w(s) by the function the kernel compiles.  Nonzero for an unknown kind, a delta that pcr_graph_set_robust_kernel
 * would refuse, or an s that is negative or not a number. */
int pcr_graph_robust_rho_w(int kind, double delta, double s, double* rho, double* w);
int pcr_graph_size(const pcr_graph* g, size_t* n_poses, size_t* n_priors, size_t* n_between);
int pcr_graph_clear(pcr_graph* g);
void pcr_graph_default_params(pcr_graph_params* p);
/* Refused with a message, before anything is solved: an id out of range; a between factor with from == to; a pose, a measurement or an
 * information matrix that is not finite; a connected component that holds neither a prior nor a fixed pose (the message names its first
 * pose); a PCR_GRAPH_HOST graph.  Duplicate edges are allowed and add up.  An empty graph returns 0 and does nothing; a graph whose poses are
 * all fixed returns 0 at once with 0 iterations, converged = 1 and chi2 evaluated; so does (0 iterations, converged = 1) a graph
 * to which nothing was added since an optimize that converged under tolerances no looser than this call's -- one that ran out of iterations
 * or of lambda, or converged under looser tolerances, goes on from the current estimates.  params == NULL: the defaults; result may be NULL.  Per trial step one launch holds the whole
 * conjugate-gradient loop (bounded on the device by pcg_max_iterations) and 24 bytes come back to the host. */
int pcr_graph_optimize(pcr_graph* g, const pcr_graph_params* params, pcr_graph_result* result);
int pcr_graph_poses(const pcr_graph* g, size_t first, size_t count, double* poses16);
/* The current estimates in device memory, *n of them, 16 doubles each (valid until the next call that adds poses or optimises); NULL on a host
 * graph.  Uploads poses added since the last use and reads no factor: it serves a graph whose factors name poses that do not exist yet. */
const double* pcr_graph_device_poses(const pcr_graph* g, size_t* n);
/* Introspection: every factor linearised at the current estimates, priors first, then betweens, each in the order added: r [E][6],
 * j_from = dr/d(delta_from) and j_to = dr/d(delta_to) [E][36] row-major (a prior's j_from is zero), unweighted for every factor, switched
 * off or not, between fixed poses or not; *chi2 = sum rho over the factors that are on.  Any pointer may be NULL.
 * A device graph runs the optimiser's kernel, a PCR_GRAPH_HOST graph the same code on the host: the two agree bit for bit. */
int pcr_graph_linearize(pcr_graph* g, double* r, double* j_from, double* j_to, double* chi2);
/* Introspection (device graphs): y = (H + lambda I) x at the current estimates, x and y 6 doubles per pose, by the solve kernel's own product.
 * H is the solve's: a fixed pose's rows and columns are lambda I (y_p = lambda x_p exactly, and x_p reaches no other row). */
int pcr_graph_apply(pcr_graph* g, double lambda, const double* x, double* y);
/* Introspection (host code only; serves a PCR_GRAPH_HOST graph): the spanning forest PCR_GRAPH_PRECOND_TREE would use.  parent[p] = the parent
 * pose of p, -1 for a root (the lowest-numbered pose of its component that holds a prior or is fixed); n = the entries parent has room for, at least the
 * number of poses (parent may be NULL, then only the counts are written).  *n_tree_edges between factors are in the forest, *n_other_edges are
 * not (loops, duplicates of a tree edge).  Refuses what pcr_graph_optimize refuses of the graph itself. */
int pcr_graph_tree(const pcr_graph* g, int64_t* parent, size_t n, size_t* n_tree_edges, size_t* n_other_edges);
/* Introspection (device graphs): z = M^-1 r at the current estimates, kind = one of PCR_GRAPH_PRECOND_*, r and z 6 doubles per pose, by the
 * factorisation and the sweeps the solve runs.  lambda >= 0; 0 is legal when every pose has a factor and none is fixed (a fixed pose's block
 * of M is lambda I: z_p = r_p / lambda, coupled to nothing).  Nonzero with a message when a block is not positive definite. */
int pcr_graph_precondition(pcr_graph* g, double lambda, int kind, const double* r, double* z);
/* Poses first .. first+count-1 of the graph become the poses of key frames first .. first+count-1 of the store, read from the graph's device
 * memory.  The store keeps its pose table on the HOST (beside the key frames' offsets), so this is one device-to-host copy inside the library,
 * not a device-to-device one; what it spares is the caller's buffer and second call.  The bits pcr_map_set_poses would store from pcr_graph_poses, with its rules (a parent, not a view; no generation moves).  Refused
 * when the two are on different devices (a host graph is on none) or when either holds fewer than first + count entries. */
int pcr_map_set_poses_from_graph(pcr_map* m, const pcr_graph* g, size_t first, size_t count);
/* g2o text files: VERTEX_SE3:QUAT and EDGE_SE3:QUAT as Backend::Gtsam::myReadG2o reads them (Backend.cpp:148-193): vertex ids consecutive
 * (continuing the graph's), the information matrix mirrored to both triangles, its translation and rotation blocks swapped into [omega; v]
 * order and its off-diagonal blocks taken as they stand (not transposed, as there); the PRIOR preset is added on vertex 0.  VERTEX3 and EDGE3
 * are refused with a message; a FIX record (g2o's convention: "FIX id", one or more ids) fixes those vertices and is refused when the file
 * defines no vertex of that id (the reference's reader ignores such records); other records are skipped.  A file that is refused leaves the
 * graph as it was.  save writes the poses, one FIX record per fixed pose after them, and the
 * between factors with 17 significant digits (no priors: they are the reader's own).  The files carry neither robust marks nor switches: save
 * writes every between factor, switched off or not, and a loaded graph has every factor on and unmarked. */
int pcr_graph_load_g2o(pcr_graph* g, const char* path);
int pcr_graph_save_g2o(const pcr_graph* g, const char* path);

/* The NDT optimiser on its own (host only, no GPU): pclomp's computeTransformation + computeStepLengthMT (ndt_omp_impl.hpp:81-171,
 * 735-932) as the state machine that pcr_scan2map runs on the device (csrc/ndt_opt.h), driven from outside -- the caller evaluates what
 * it asks for and feeds the 43 sums back.  An introspection entry point like pcr_ndt_derivatives: the CPU test suite drives it with the
 * oracle's derivatives and must arrive where the oracle's own loop arrives.
 *   request: kind 0 = score + gradient + Hessian at p6 (computeDerivatives), 1 = score + gradient only, 2 = computeHessian (double) at
 *            the same p6 as the previous request, 3 = finished.  (Score + gradient are never asked for twice running at one p6: the
 *            reference's clamped trial steps do repeat, and the state machine feeds itself the sums it already has.)  pose16 (optional) = the float transform of p6, column-major.
 *   feed:    sums = score, gradient[6], Hessian[36] (row-major; ignored entries may be anything finite).
 *   result:  the pose computeTransformation would return (Matrix4f values), converged flag, iterations. */
typedef struct pcr_ndt_opt pcr_ndt_opt;
pcr_ndt_opt* pcr_ndt_opt_create(const double pose_guess[16], double step_size, double trans_eps, int max_iters);
void pcr_ndt_opt_destroy(pcr_ndt_opt* o);
int pcr_ndt_opt_request(const pcr_ndt_opt* o, int* kind, double p6[6], double pose16[16]);
int pcr_ndt_opt_feed(pcr_ndt_opt* o, const double sums[43]);
int pcr_ndt_opt_result(const pcr_ndt_opt* o, double pose16[16], int* converged, int* iterations, int* done);
/* evaluations = computeDerivatives calls of the reference's loop so far, hessians = its computeHessian calls, replayed = how many of the
 * evaluations were requests for score + gradient at the point they had just been evaluated at, answered without asking (ndt_opt.h) */
int pcr_ndt_opt_counts(const pcr_ndt_opt* o, int* evaluations, int* hessians, int* replayed);
/* pcr_ndt_opt_set_replay (before the first feed): off != 0 = every request becomes an evaluation, the reference's own schedule
 * (pcr_params.ndt_evaluate_repeats); the decisions and the result must not depend on it.
 * pcr_ndt_opt_create_device: the same object with its state in device memory: every feed uploads the sums and launches the controller
 * step of the sharded device loop once (one block; the Newton solve is the device's guarded elimination, the trigonometry the device's),
 * request / result / counts / state / tables read the copy that launch left.  NULL when there is no GPU.
 * pcr_ndt_opt_state: bail = the device's Newton solve met a pivot below its guard and ended the run for the host to repeat (then done = 1,
 * kind 3); late_h = Hessians asked for at a first trial point after the search had ended there; a_t = the current trial step;
 * phase = ndt_opt.h's kNdtPhase*.  pcr_ndt_opt_tables: the angle tables of the request (computeAngleDerivatives: j_ang, h_ang as float,
 * j_ang_a_.. and h_ang_a2_.. as double, row-major [8][3] / [15][3]).  pcr_ndt_opt_hessian: the 36 Hessian entries the state keeps. */
pcr_ndt_opt* pcr_ndt_opt_create_device(const double pose_guess[16], double step_size, double trans_eps, int max_iters);
int pcr_ndt_opt_set_replay(pcr_ndt_opt* o, int off);
int pcr_ndt_opt_state(const pcr_ndt_opt* o, int* bail, int* late_h, double* a_t, int* phase);
int pcr_ndt_opt_tables(const pcr_ndt_opt* o, float j[24], float h[45], double jd[24], double hd[45]);
int pcr_ndt_opt_hessian(const pcr_ndt_opt* o, double hess[36]);

/* The VGICP optimiser on its own (host only, no GPU): fast_gicp's LsqRegistration::computeTransformation + step_lm
 * (lsq_registration_impl.hpp:53-79, 125-171) as the state machine that pcr_scan2map runs on the device (csrc/vgicp_opt.h), driven
 * from outside like pcr_ndt_opt_*: the caller evaluates what it asks for and feeds the 29 sums back.
 *   request: kind 0 = linearize at pose_eval (fast_vgicp_impl.hpp:119-180); 1 = an LM trial: compute_error (:183-204) at pose_eval on
 *            the correspondences of the linearisation at pose_lin, AND the linearisation at pose_eval; 2 = finished.  Poses column-major.
 *   feed:    sums = H upper triangle row by row (21), b (6), error of the linearisation at pose_eval (1), the trial's error (1).
 *   result:  the pose computeTransformation would return (before the Matrix4f cast of VgicpRegister.cpp:37), converged, outer iterations. */
typedef struct pcr_vgicp_opt pcr_vgicp_opt;
pcr_vgicp_opt* pcr_vgicp_opt_create(const double pose_guess[16], int max_iters, int lm_inner, double lm_init_scale, double rot_eps, double trans_eps);
void pcr_vgicp_opt_destroy(pcr_vgicp_opt* o);
int pcr_vgicp_opt_request(const pcr_vgicp_opt* o, int* kind, double pose_eval[16], double pose_lin[16]);
int pcr_vgicp_opt_feed(pcr_vgicp_opt* o, const double sums[29]);
int pcr_vgicp_opt_result(const pcr_vgicp_opt* o, double pose16[16], int* converged, int* outer_iterations, int* done);

/* Profiling aid: with pcr_params.record_timeline = 1 thread 0 of every linearisation block records seven
 * s_memrealtime stamps (100 MHz ticks): entry, prologue done, misses posted, search done, plane+cache done,
 * accumulation done, partial sums stored (+ the fold inside the prologue, three stamps of the dense search and the stamps inside
 * the refine, post and accumulate stages: LoamRegister.timeline in pcr.py lists the columns).  out receives
 * [launches][blocks][24] u64; call with out = NULL to size it. */
int pcr_get_timeline(pcr_handle* h, uint64_t* out, size_t capacity, int* launches, int* blocks);

/* NDT introspection: one computeDerivatives pass (ndt_omp_impl.hpp:180-285) at the parameter vector
 * p = [tx ty tz, roll pitch yaw] (Translation * Rx * Ry * Rz, ndt_omp_impl.hpp:146-149) against the current
 * target (pcr_set_target): score, gradient (6), Hessian (36, row-major) and, when hess_d != NULL, the
 * double-precision Hessian of computeHessian (ndt_omp_impl.hpp:541-645) at the same pose. */
int pcr_ndt_derivatives(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device,
                        const double p[6], double* score, double grad[6], double hess[36], double* hess_d);

/* NDT introspection: the voxel Gaussians of the current target (pcr_set_target), one record per voxel that was kept
 * (VoxelGridCovariance::Leaf, voxel_grid_covariance_omp_impl.hpp:49-370): ijk = the voxel's lattice coordinates floorf(p * inverse_leaf)
 * (not relative to the box's min_b), n = its points, mean, icov (row-major).  In no particular order.
 * *count = the voxels kept, *rejected = the cells that had at least max(3, ndt_min_points) points but failed the eigenvalue or the
 * inverse test (:337-341, :359-364).  out = NULL sizes the call; with out, capacity (in records) must be at least *count.
 * A handle whose target pcr_scan2map prepared for that one scan's region only is refused: call pcr_set_target first. */
typedef struct pcr_ndt_voxel {
    int32_t ijk[3];
    int32_t n;
    double mean[3];
    double icov[9];
} pcr_ndt_voxel;
int pcr_ndt_voxels(pcr_handle* h, pcr_ndt_voxel* out, size_t capacity, size_t* count, size_t* rejected);
/* VGICP introspection (a vgicp handle): the Gaussian voxels of the kept target (pcr_set_target) as the fold left them
 * (fast_vgicp_voxel.hpp:79-174, pcr_params.vgicp_voxel_mode), one record per voxel: ijk = the voxel's lattice coordinates floor(p / res - 0.5)
 * (:158-160), n = its points, mean, cov = xx xy xz yy yz zz.  In no particular order.  *count = the voxels; out = NULL sizes the call; with
 * out, capacity (in records) must be at least *count.  A handle whose target pcr_scan2map prepared for that one scan's region only is
 * refused: call pcr_set_target first. */
typedef struct pcr_vgicp_voxel {
    int32_t ijk[3];
    int32_t n;
    double mean[3];
    double cov[6];
} pcr_vgicp_voxel;
int pcr_vgicp_voxels(pcr_handle* h, pcr_vgicp_voxel* out, size_t capacity, size_t* count);
/* VGICP introspection: the pairs of the LAST pcr_vgicp_linearize on this handle (pcr_params.vgicp_search), one record per pair: row = the source
 * point's row, ijk = the voxel's lattice coordinates (as pcr_vgicp_voxel's).  Ordered by row, a row's pairs in the order of the setting's table.
 * *count = the pairs (pcr_vgicp_linearize's n_corr); out = NULL sizes the call; with out, capacity (in records) must be at least *count. */
typedef struct pcr_vgicp_corr {
    int32_t row;
    int32_t ijk[3];
} pcr_vgicp_corr;
int pcr_vgicp_correspondences(pcr_handle* h, pcr_vgicp_corr* out, size_t capacity, size_t* count);
/* NDT introspection: the sums of one pass as the device-resident loop of pcr_scan2map / pcr_align computes and folds them (one launch
 * per pass, the fold in the prologue of the next launch) -- where pcr_ndt_derivatives runs the kernels of the host-driven loop.  The
 * loop's own two launches on a state that asks for one pass at p and ends: the sums are read from the state the second launch hands on.
 *   kind 0: score, gradient, float Hessian (computeDerivatives)   1: score and gradient only (a line-search pass; hess = 0)
 *        2: the double Hessian of computeHessian (score = 0, grad = 0)
 * Handles without a communicator only (a tile set with pcr_set_shard is honoured). */
int pcr_ndt_pass_sums(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double p[6], int kind,
                      double* score, double grad[6], double hess[36]);

int pcr_get_stats(pcr_handle* h, pcr_stats* out);
/* 0: no timing events; 1: phase events (default); 2: also an event pair around every
 * launch of the dominant kernel (adds host work; for roofline measurement only). */
int pcr_set_profile(pcr_handle* h, int level);
/* Use an existing HIP stream (hipStream_t) instead of the handle's own. */
int pcr_set_stream(pcr_handle* h, void* hip_stream);

/* ---- multi-GPU (one process per GPU; map tiles + 1-cell halo per rank) ---- */

/* Restrict the handle to queries whose transformed position lies in [lo, hi) (metres,
 * map frame): each scan point is then processed by exactly one rank.  lo > hi clears it. */
int pcr_set_query_tile(pcr_handle* h, const double lo[3], const double hi[3]);
/* RCCL communicator for the per-linearisation all-reduce of the normal equations
 * (28 doubles).  unique_id = 128 bytes from pcr_comm_unique_id on rank 0, shared by the
 * caller (e.g. torch.distributed broadcast).  librccl is dlopen'ed here, never before. */
int pcr_comm_unique_id(void* out128);
int pcr_comm_init(pcr_handle* h, const void* unique_id128, int rank, int nranks);
/* Who takes part in this handle's exchange: *transport = 0 none (unsharded), 1 RCCL, 2 the caller's collective, 3 the peer exchange.  With RCCL
 * rank and nranks are read back from the communicator (ncclCommUserRank / ncclCommCount), not from the arguments it was
 * created with -- bench.py reports them as "rccl_ranks". */
int pcr_comm_info(const pcr_handle* h, int* rank, int* nranks, int* transport);
/* The same exchange through a caller-supplied collective (MPI, gloo, threads of one process ...), used when no RCCL
 * communicator is set: fn must combine `count` doubles IN PLACE over all ranks -- op 0 = sum, 1 = max -- return 0 on
 * success, and leave bitwise-identical results on every rank (the ranks then solve redundantly and must agree).  It is
 * called on the thread that called the registration entry point, between device launches (one host round trip per
 * linearisation: the fallback and test path; RCCL keeps the exchange on the device).  fn == NULL clears it. */
typedef int (*pcr_allreduce_fn)(double* inout, size_t count, int op, void* user);
int pcr_comm_init_host(pcr_handle* h, pcr_allreduce_fn fn, void* user, int rank, int nranks);
/* Peer exchange (PROTOTYPE, loam handles): the ranks' 32 sums without a collective library -- every rank pushes its values into a slot of
 * every peer's receive buffer (stores over xGMI into memory mapped through hipIpc), waits for its own buffer to fill and folds the slots in
 * rank order; one small launch per linearisation instead of a reduce kernel + ncclAllReduce (csrc/loam.hip: peer_exchange_block).
 *   1. every rank: pcr_comm_peer_export(h, handle)  -> 64 bytes (a hipIpcMemHandle_t) naming its receive buffer
 *   2. the caller shares the handles (any channel: MPI, gloo, a file), in rank order
 *   3. every rank: pcr_comm_init_peer(h, handles (nranks x 64 bytes), rank, nranks)      (nranks <= 8: one node)
 * A rank that does not arrive within 2 s fails the exchange on every rank that waited for it (no device hang).  pcr_comm_info: transport 3. */
int pcr_comm_peer_export(pcr_handle* h, void* ipc_handle64);
int pcr_comm_init_peer(pcr_handle* h, const void* ipc_handles, int rank, int nranks);
/* Tile of a sharded target, all three methods: the handle processes the scan points whose transformed position lies in
 * [lo, hi) (as pcr_set_query_tile) and is promised that the target cloud it is given holds EVERY map point inside
 * [lo - halo, hi + halo) (faces at +-1e30 are open).  What the halo must cover:
 *   loam   the k-NN gate radius (sqrt(loam_knn_max_sq) = 1 m, LoamRegister.cpp:59);
 *   ndt    lo, hi multiples of ndt_resolution and halo >= one voxel (two unless the resolution is a power of two): the
 *          DIRECT7 neighbourhood (ndt_omp_impl.hpp:242) reads the six face voxels, which must be complete.  DIRECT26 needs the
 *          same (the halo extends the tile along every axis: a box that holds the edge and corner voxels too), DIRECT1 one
 *          voxel less (none at a power-of-two resolution); the refusal names the pcr_params.ndt_search in force;
 *   vgicp  lo, hi on the voxel lattice ((k + 0.5) * vgicp_resolution, fast_vgicp_voxel.hpp:158-160) and a halo that holds
 *          the 20 nearest neighbours of every point of the tile (fast_gicp_impl.hpp:253): checked on the device for every
 *          point within one voxel of the tile -- a neighbourhood that reaches past the halo fails the call on all ranks.
 *          pcr_params.vgicp_search must be PCR_VGICP_DIRECT1: under DIRECT7 / DIRECT27 a neighbour voxel may belong to another rank's tile, and
 *          pcr_set_shard, pcr_comm_init* and pcr_set_params refuse the combination with a message that names the setting.
 * Misaligned bounds are refused.  lo[0] > hi[0] clears the tile. */
int pcr_set_shard(pcr_handle* h, const double lo[3], const double hi[3], double halo);

/* Replace the parameters of a live handle (host-side state; the prepared target is dropped when a parameter that shaped
 * it changed).  VgicpRegister::initForLC() (PCR/src/VgicpRegister.cpp:21-28, called on a constructed object at
 * backend/src/LoopClosureManager.cpp:21-22) = pcr_set_params with vgicp_max_iters 100, vgicp_trans_eps 1e-6.  device and
 * struct_size must match the handle's. */
int pcr_set_params(pcr_handle* h, const pcr_params* p);
int pcr_get_params(const pcr_handle* h, pcr_params* out);

/* The fitness score of the reference's test/align.cpp:29-61: the source transformed by `pose` (float, as
 * pcl::transformPointCloud), 1-NN in the handle's current target, mean of the squared distances that are <= max_sq
 * (align.cpp uses 1.0); *n_in = points counted.  score = -1 when none is (align.cpp:56-59).  Any method's handle with a target.
 * The distances are float, bit for bit PCL's, and the gate is the comparison in double (a float distance against max_sq): *n_in is
 * exact, and the score differs from a brute-force one only by the order of the double sum.  Source points with a coordinate that is
 * not finite are not counted.
 * A handle whose last pcr_scan2map indexed the scan's region only (pcr_stats.region_index): VGICP searches its covariance search grid,
 * which holds every point; NDT indexes the target again, in full, when that target came in as a HOST buffer (it still lies in the
 * handle's staging copy); a DEVICE target is the caller's and may be gone: the call fails and says so (pcr_set_target, or
 * pcr_params.full_target = 1, avoid it).
 * An index cut to a region (a target too spread out for the dense tables: its bulk, or the room around a scan): when a source point's
 * nearest indexed point is not provably nearer than the cut faces (and than the gate), the dense index cannot answer, and the score is
 * taken again on the SPARSE index of the kept target (below, at the neighbour queries: built by the first call that needs it, kept until
 * the target changes), which holds every point: the same float distances, the same gate, the sums in the same order -- the number the
 * dense index would have given had it held the whole target.  It never returns the score of the part that was indexed.  Where the sparse
 * index cannot be had -- the target was a caller's device buffer that the handle did not copy (pcr_scan2map_device, pcr_scan2map_submap),
 * or its cell box needs more than 63 key bits -- the call fails as it used to: score = -1, *n_in = 0, and the message names the cut and
 * then the sparse index's reason.
 * pcr_params.query_index governs the scores as it governs the queries: under PCR_QUERY_INDEX_SPARSE pcr_fitness, pcr_fitness_gated,
 * pcr_fitness_batch and the scores of pcr_relocalize / pcr_relocalize_global always run on the sparse index (a handle of any method; bit
 * for bit the dense index's scores wherever that one answers); under AUTO they run on the dense index as ever, with the same launches, and
 * go to the sparse one only for what a cut dense index refuses.  Sharded handles and handles with a query tile are not served by the
 * sparse index: their refusals stand.  pcr_query_index_info says which index answered the last score. */
int pcr_fitness_gated(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double pose[16],
                      double max_sq, double* score, int64_t* n_in);

/* ---- Neighbour queries on the kept target ---------------------------------------------------------------------------------------------
 * The two operations of the reference's spatial index, nanoflann::PointCloudKdtree (third_parties/nanoflann/include/nanoflann/
 * pcl_adaptor.hpp:47-78: nearestKSearch, radiusSearch), asked of the index this library keeps in HBM: the handle's kept target
 * (pcr_set_target, or a host target of pcr_scan2map), on a handle of any method, always over the FULL cloud (a target that the last
 * pcr_scan2map prepared for its scan's region only is prepared in full first, as pcr_align does).
 * Semantics: float coordinates widened to double, d2 = dx*dx + dy*dy + dz*dz in double, added in that order -- the reference's
 * metric_L2_Simple with Scalar = double, bit for bit.  idx is a point's position in the cloud the target was set from; points with a
 * coordinate that is not finite are not indexed and do not renumber the others.  Results ascend by (d2, idx): ties go to the lower
 * index (nanoflann's tie order follows its tree walk and is not reproduced).
 * queries: n_q records of stride_bytes (x, y, z floats first; 16 or 32 bytes in the reference's clouds), host or device memory.  The
 * outputs are host arrays.  Neither call changes what a later registration computes.  Sharded handles and handles with a query tile
 * are refused with a message.
 * A target whose box cannot be tabulated (two sessions 30 km apart, one stray return kilometres off: the registrations cut the dense
 * index to the bulk of the cloud) is answered from the SPARSE index: the points sorted by a 64-bit cell key (1 m cells, z then y then x,
 * each axis a power-of-two field) and nothing else -- 24 bytes per point whatever the box, every row of cells found by binary search.
 * pcr_params.query_index = PCR_QUERY_INDEX_SPARSE asks for it on every target; the answers are the dense index's bit for bit.  It is built
 * by the first query that needs it after the target was set, from the handle's OWN copy of the target's points (pcr_set_target copies
 * host and device buffers alike; a host target of pcr_scan2map lies in the handle's staging area) -- never from a caller's device
 * buffer, which may be gone by then: after pcr_scan2map_device or pcr_scan2map_submap the sparse index is refused with a message
 * that says so -- and kept until the target changes (pcr_set_target, pcr_scan2map*, pcr_invalidate_target, a pcr_set_params that
 * drops the target, pcr_destroy).  AUTO goes by the dense index's own mark of a cut: a handle whose LAST target was cut may take that
 * target's box over as the hint of its next index, and the mark with it, so that a compact target set on the same handle is answered
 * from the sparse index too (exactly; before, it was refused) -- a fresh handle, or pcr_params.index_no_hints, answers it from the dense one.
 * Refused, with the three extents in the message: a cloud whose cell box needs more than 63 key
 * bits, or has a cell number of 2^62 or beyond (a stray point at 3e38 m); the handle stays usable. */
#define PCR_KNN_MAX_K 32

/* The k nearest target points of every query, 1 <= k <= PCR_KNN_MAX_K, with no range gate.  Row q of idx / d2 (k entries) ascends by
 * (d2, idx); when the target holds fewer than k points, and for a query with a coordinate that is not finite, the rest of the row is
 * idx = -1, d2 = +inf. */
int pcr_knn(pcr_handle* h, const void* queries, size_t n_q, size_t stride_bytes, int on_device, int k, int64_t* idx, double* d2);

/* The target points with d2 < radius * radius (strict, the square taken in double: RadiusResultSet::addPoint, pcl_adaptor.hpp:65) of
 * every query; radius finite and > 0.  Query q's results are idx / d2 [offsets[q], offsets[q + 1]); offsets (n_q + 1 entries) and
 * *n_total = offsets[n_q] are written whenever the search itself ran, and the counts are exact.  capacity: entries idx and d2 hold.
 * capacity < *n_total: nothing is written to idx / d2, the call returns 1 with a message that names both numbers, and the caller
 * sizes the arrays and calls again (the pcr_reloc_hypotheses pattern; idx and d2 may be NULL when capacity is 0).
 * sorted = 1: every segment ascends by (d2, idx).  sorted = 0: the order inside a segment is unspecified.
 * A query with a coordinate that is not finite has no results. */
int pcr_radius_search(pcr_handle* h, const void* queries, size_t n_q, size_t stride_bytes, int on_device, double radius, int sorted,
                      size_t capacity, uint64_t* offsets, int64_t* idx, double* d2, size_t* n_total);

/* Which index answered the last pcr_knn / pcr_radius_search or the last fitness score (pcr_fitness, pcr_fitness_gated, pcr_fitness_batch,
 * the scores of a relocalisation) of the handle: *kind = PCR_QUERY_INDEX_DENSE or PCR_QUERY_INDEX_SPARSE (-1: none has been answered
 * since the target was set; a batch says SPARSE when any of its poses went there), *n_points = the points it holds (the finite ones),
 * *bytes = the device memory it occupies (dense: the sorted points and the cell table; sparse: 24 bytes per point).  Any pointer may be NULL. */
int pcr_query_index_info(pcr_handle* h, int* kind, size_t* n_points, size_t* bytes);

/* ---- Relocalisation from a coarse pose ----------------------------------------------------------------------------------------------
 * The caller: the localisation program's operator sets the robot's pose by a click (/initialpose, dataproxy/src/RelocDataProxy.cpp:34-48)
 * and LidarOdometry::generateOdom takes that click as the initial guess of ONE scan2Map (frontend/src/LidarOdometry.cpp:67-77, 121-126,
 * 184).  A click is off by a metre or more and 10-30 degrees of yaw, outside the basin of convergence of LOAM, NDT and VGICP.
 * pcr_relocalize scores a lattice of (x, y, yaw) hypotheses around it, refines the best few and keeps the one that fits best. */

/* The most poses one pcr_fitness_batch or pcr_reloc_hypotheses call takes (2^20), and the most source points it scores per pose (2^26). */
#define PCR_RELOC_MAX_POSES 1048576u
#define PCR_BATCH_MAX_POINTS 67108864u

/* pcr_fitness_gated for K poses (16 doubles each, column-major, host memory) of one source in one pass.  For every pose k, scores[k] and
 * n_in[k] are what pcr_fitness_gated returns for that pose: *n_in exact, the score that of another summation order at most.  For a
 * subset of up to 131 072 points the sum is taken in pcr_fitness_gated's own order: the results are bit for bit the single-pose call's.
 * Two calls return identical bytes (no atomics).
 * score_points: 0, or a value >= n_src, scores every point; otherwise the points i_j = floor(j n_src / score_points) (64-bit integer
 * arithmetic), j = 0 .. score_points - 1, indexed on the device in place.
 * The index searched is pcr_fitness_gated's (a region-only lattice: VGICP's covariance grid, or an NDT host target indexed again).
 * An index cut to a region: exactly the poses with a point whose nearest target point the dense index cannot prove are scored again on
 * the sparse index (pcr_fitness_gated's rule; bit for bit its result, whichever index answered either).  Only where the sparse index cannot
 * be had do they get scores[k] = -1, n_in[k] = -1 (where pcr_fitness_gated fails); the others are scored, and the call returns 0.
 * K <= PCR_RELOC_MAX_POSES, and at most PCR_BATCH_MAX_POINTS points are scored per pose (n_src, or score_points when it is smaller;
 * more is refused with a message).  Sharded handles and handles with a query tile (pcr_set_query_tile) are refused. */
int pcr_fitness_batch(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const double* poses, size_t K,
                      double max_sq, size_t score_points, double* scores, int64_t* n_in);

typedef struct pcr_reloc_params {
    uint32_t struct_size;         /* sizeof(pcr_reloc_params), set by pcr_reloc_default_params */
    double xy_range, xy_step;     /* half-width and step of the x and y search, m (default 2, 0.5) */
    double yaw_range, yaw_step;   /* half-width and step of the yaw search, rad (default 30 and 5 degrees) */
    double max_sq;                /* gate of both scores (the reference's test/align.cpp: 1.0) */
    int32_t refine_top;           /* distinct coarse winners refined by the handle's method (default 4) */
    int32_t pad_;
    uint64_t score_points;        /* source subset of the coarse score (pcr_fitness_batch; default 4096) */
} pcr_reloc_params;
void pcr_reloc_default_params(pcr_reloc_params* p);

/* The hypothesis lattice around `coarse` (no device work).  nx = floor(xy_range / xy_step + 1e-9), nk = floor(yaw_range / yaw_step + 1e-9)
 * (0 for a zero range).  Hypothesis (i, j, k), i, j in [-nx, nx], k in [-nk, nk], is number h = ((k + nk)(2nx + 1) + (j + nx))(2nx + 1) + (i + nx)
 * (yaw outermost, then y, then x); its pose: translation t_c + (i xy_step, j xy_step, 0), rotation Rz(k yaw_step) R_c (about the map's z
 * axis through the sensor), row by row with c = cos, s = sin (C library, double): row0 = c R0 - s R1, row1 = s R0 + c R1, row2 = R2.
 * poses: capacity x 16 doubles; *K = the number written.  Refused with a message (pcr_last_error(NULL)): a non-positive step with a
 * nonzero range, K > PCR_RELOC_MAX_POSES, refine_top < 1, a NULL or too small output. */
int pcr_reloc_hypotheses(const double coarse[16], const pcr_reloc_params* p, double* poses, size_t capacity, size_t* K);

typedef struct pcr_reloc_candidate {
    int64_t hypothesis;           /* lattice number h of the pose the refinement started from */
    int64_t coarse_n_in;          /* its coarse score (the score_points subset) */
    double coarse_score;
    double pose[16];              /* the refined pose (pcr_align from the hypothesis) */
    int32_t converged;
    int32_t pad_;
    int64_t n_in;                 /* the refined pose's score on the whole source */
    double score;
} pcr_reloc_candidate;

/* Relocalise: the preconditions of pcr_align (a kept target).  1. every hypothesis of pcr_reloc_hypotheses(pose_inout) is scored by
 * pcr_fitness_batch on the score_points subset; 2. they are ranked by (-n_in, score, h), ascending, leaving out those with n_in <= 0 or
 * refused; 3. down the ranking a hypothesis is taken unless one taken already lies within 1 of it in each of i, j and k (no yaw wrap),
 * until refine_top are; 4. the click itself (0, 0, 0) is added when it was not taken; 5. each candidate is refined by pcr_align from its
 * hypothesis pose -- bit for bit pcr_align's result; 6. the refined poses are scored on the WHOLE source (pcr_fitness_batch) and the
 * first by (-n_in, score, candidate order) is chosen; 7. it is written to pose_inout / *converged, every candidate to cands (in the order
 * taken, the click last when it was added) and the chosen one's index to *chosen.
 * Fails (with a message) when no hypothesis has a point within the gate (a click far off the map), when a refinement fails (not
 * converging is no failure), when capacity < refine_top + 1, or when n_src > PCR_BATCH_MAX_POINTS (the final score covers every point).
 * State of the handle afterwards: pcr_fitness() (VGICP's getFitnessScore) evaluates the CHOSEN pose -- what it returns after a pcr_align
 * from the chosen hypothesis.  pcr_get_stats, pcr_get_trace and pcr_get_timeline describe the last refinement, i.e. candidate
 * *n_cands - 1 (the click when it was added), not necessarily the chosen one. */
int pcr_relocalize(pcr_handle* h, const void* src, size_t n_src, size_t stride_bytes, int on_device, const pcr_reloc_params* p,
                   double pose_inout[16], int* converged, pcr_reloc_candidate* cands, size_t capacity, size_t* n_cands, size_t* chosen);

/* ---- Global relocalisation: no pose at all (start-up, or tracking lost) ----------------------------------------------------------------
 * The places are the key frames whose ScanContext is nearest the scan's (pcr_sc_distances against every stored context); around each
 * place's coarse pose a pcr_relocalize lattice is scored, all places in one pass, and the best refined pose is chosen. */
typedef struct pcr_global_reloc_params {
    uint32_t struct_size;      /* set by pcr_global_reloc_default_params */
    int32_t places;            /* best contexts tried, by (dist, id) ascending (default 5) */
    double max_dist;           /* contexts with dist > max_dist are not tried (default DBL_MAX: no limit) */
    pcr_reloc_params local;    /* lattice around each place, gate, refine_top PER PLACE, score_points;
                                  default +-2 m @ 0.5 m, +-9 deg @ 3 deg, refine_top 2, max_sq 1, 4096 points */
} pcr_global_reloc_params;
void pcr_global_reloc_default_params(pcr_global_reloc_params* p);

typedef struct pcr_global_reloc_candidate {
    int64_t place;             /* context / key-frame index */
    double sc_dist; int32_t sc_shift; int32_t pad_;
    pcr_reloc_candidate c;     /* hypothesis (within that place's lattice), coarse and final scores, refined pose */
} pcr_global_reloc_candidate;

/* Host-only (no device work): the coarse pose of a place, kf_pose * Rz(-yaw) with yaw = deg2rad<float>(6 * shift) as pcr_sc_query forms
 * it -- the rotation about the key frame's own z: with c = cos(yaw), s = sin(yaw) (C library, double), column 0 becomes c C0 - s C1 and
 * column 1 becomes s C0 + c C1 -- and its pcr_reloc_hypotheses lattice (capacity x 16 doubles, *K = the number written).  Refused with a
 * message (pcr_last_error(NULL)) as pcr_reloc_hypotheses refuses. */
int pcr_global_reloc_hypotheses(const double kf_pose[16], int32_t shift, const pcr_reloc_params* local,
                                double* poses, size_t capacity, size_t* K);

/* Global relocalisation: the preconditions of pcr_relocalize (a kept target, e.g. the whole map; no shards, no query tile), and a
 * ScanContext database on the handle's device with one context per key frame, kf_poses its n_kf = pcr_sc_size() poses (16 doubles
 * each, column-major).  1. pcr_sc_distances of src (the registration's own cloud, sensor frame); the places are the best p->places
 * contexts by (dist, id), leaving out those at DBL_MAX or beyond max_dist; 2. every place's pcr_global_reloc_hypotheses lattice, all
 * places in ONE pcr_fitness_batch pass on the score_points subset; 3. per place, ranking and distinct winners exactly as steps 2-3 of
 * pcr_relocalize (no click is added); 4. each candidate refined by pcr_align from its hypothesis pose (bit for bit pcr_align), the
 * refined poses scored on the whole source in one pass, and the first by (-n_in, score, candidate order) chosen -- candidate 0 when
 * none has a point in the gate.  Candidates are ordered by place rank, then in the order taken; capacity >= places * local.refine_top.
 * Fails with a message, the handle untouched, when no place qualifies or no hypothesis of any place has a point within the gate.
 * The handle afterwards: as after pcr_relocalize (pcr_fitness() evaluates the chosen pose).  Refused parameters and outputs are reported
 * through pcr_last_error(h), or pcr_last_error(NULL) when h is NULL. */
int pcr_relocalize_global(pcr_handle* h, pcr_sc* sc, const double* kf_poses, size_t n_kf, const void* src, size_t n_src, size_t stride_bytes,
                          int on_device, const pcr_global_reloc_params* p, double pose_out[16], int* converged,
                          pcr_global_reloc_candidate* cands, size_t capacity, size_t* n_cands, size_t* chosen);

/* ---- The front end's per-scan loop -----------------------------------------------------------------------------------------------------
 * LidarOdometry::handler / generateOdom reduced to what touches the registration (frontend/src/LidarOdometry.cpp:160-214,
 * frontend/src/MapManager.cpp:109-201), strung together once, in the library: scan -> voxel filter -> scan2Map against the sub-map ->
 * SixDof2Mobile -> setCurPose -> putKeyFrame -> updateMap.  simpleslam_amd/sequence.py's drive() over GpuFront is the same loop in Python,
 * and the two are pinned to each other bit for bit. */

/* Host only (no GPU): trans::SixDof2Mobile (common/geometry/trans.hpp:68-86), which LidarOdometry applies to every refined pose
 * (LidarOdometry.cpp:211), in Eigen's order of operations.  The rotation goes to a quaternion (Eigen's Quaternion(Matrix3): the trace
 * branch, or the branch of the largest diagonal element), the quaternion to an angle and an axis (AngleAxis(Quaternion): n = |(x, y, z)|,
 * angle = 2 atan2(n, |w|), axis = (x, y, z) / (w < 0 ? -n : n); n == 0: angle 0, axis (1, 0, 0)).  The result has the translation
 * (tx, ty, 0), tx and ty copied, and the rotation by `angle` about copysign(1, axis.z) * Z when |axis.z| > 0.95: R00 = R11 = cos,
 * R01 = -a sin, R10 = a sin, R22 = (1 - cos) + cos.  Otherwise -- a rotation mostly about another axis -- the rotation is the identity:
 * THE HEADING IS DROPPED, as the reference drops it.  NULL arguments return nonzero; out may alias T. */
int pcr_pose_to_mobile(const double T[16], double out[16]);

typedef struct pcr_frontend pcr_frontend;
typedef struct pcr_frontend_params {
    double grid_size;   /* downSampleVoxelGridSize, default 0.5: scan filter and sub-map filter */
    double radius;      /* mSurroundingKeyframeSearchRadius, default 8.0 */
    double kf_gap;      /* minKFGap, default 1.0 */
    int32_t mobile;     /* 1: pcr_pose_to_mobile on every refined pose (LidarOdometry.cpp:211); default 0 */
} pcr_frontend_params;
typedef struct pcr_frontend_info {
    int32_t registered;      /* 0: the sub-map was empty, the pose is the initial one */
    int32_t converged, iterations;
    int32_t keyframe_added, update_queued;
    int64_t n_filtered, n_submap;        /* filtered scan; sub-map this scan was registered against */
    int64_t keyframes, updates;          /* totals so far */
    double seconds[5];                   /* host time of this step: voxel, wait, scan2map, add_keyframe, update_map */
} pcr_frontend_info;

void pcr_frontend_default_params(pcr_frontend_params* p);
/* Borrows both: `reg` (any method) and `map` (a parent, not a view) must outlive the front end and are used by nobody else while a step
 * runs.  p == NULL uses the defaults.  NULL on failure; pcr_frontend_last_error(NULL) then holds the reason. */
pcr_frontend* pcr_frontend_create(pcr_handle* reg, pcr_map* map, const pcr_frontend_params* p);
void pcr_frontend_destroy(pcr_frontend* fe);
const char* pcr_frontend_last_error(const pcr_frontend* fe);   /* fe == NULL: the last create failure */
/* One scan.  init_pose: where the scan is expected (the caller's generateOdom: previous pose o odometry; the front end composes nothing).
 *   1. the scan is voxel-filtered at grid_size into a device buffer of the front end's -- or, when pcr_frontend_prefetch queued exactly this
 *      scan (same pointer, n and stride), that filter is collected;
 *   2. a queued sub-map assembly is collected: n_submap = the sub-map this scan meets;
 *   3. n_submap > 0: pcr_scan2map_submap from init_pose (converged, iterations: the handle's).  Otherwise the pose is init_pose,
 *      converged = 1, iterations = 0, registered = 0;
 *   4. params.mobile: pcr_pose_to_mobile of the pose, whether or not a registration ran;
 *   5. setCurPose (MapManager.cpp:109-119): an assembly is due when none has happened yet or |last_update - t| > kf_gap;
 *   6. putKeyFrame (:121-149): the RAW scan becomes a key frame under the pose when there is none yet or the smallest SQUARED distance
 *      from t to a key-frame position is > kf_gap (squared distance against the gap itself, as the reference has it).  Positions are
 *      kept on the host, in double, (dx^2 + dy^2) + dz^2;
 *   7. when an assembly is due: pcr_map_update_begin(t, radius, grid_size) -- queued, collected by step 2 of the next scan (its kernels
 *      run beside that scan's filter, as the reference's map thread works beside its front end) or by pcr_frontend_finish.
 * LidarOdometry::selectKeyFrame's own gate (LidarOdometry.cpp:80-87) is NOT applied: every scan is offered to putKeyFrame.
 * scan: n > 0 records of stride_bytes, host or device memory; a host scan is uploaded first.  It must stay untouched until the step returns.
 * Nonzero on failure, the inner call's message prefixed by the step's name; a queued assembly that failed is reported by the step (or
 * the pcr_frontend_finish) that collects it.  After a failed step the loop's state is what the completed parts left; pcr_frontend_reset
 * starts over.  info may be NULL. */
int pcr_frontend_step(pcr_frontend* fe, const void* scan, size_t n, size_t stride_bytes, int on_device,
                      const double init_pose[16], double pose_out[16], pcr_frontend_info* info);
/* One scan of a moving sensor: pcr_deskew (above; on the register's handle) of the scan into a device buffer of the front end's own, then exactly
 * pcr_frontend_step(on_device = 1) on that buffer -- the key frame of step 6 is therefore the DESKEWED scan.  The caller supplies the motion as it
 * supplies init_pose: the front end composes nothing.  A filter queued by pcr_frontend_prefetch is collected and dropped (timed scans are not
 * prefetched).  A refusal of the deskew comes back under "deskew: " and leaves the loop's state as it was.  dinfo may be NULL. */
int pcr_frontend_step_timed(pcr_frontend* fe, const void* scan, size_t n, size_t stride_bytes, int on_device, const void* times, int time_kind,
                            long long time_offset_bytes, const pcr_deskew_motion* m, const double init_pose[16], double pose_out[16],
                            pcr_frontend_info* info, pcr_deskew_info* dinfo);
/* Queue the voxel filter of a scan that is registered LATER (pcr_voxel_filter_begin on a second handle of the front end's own, on the
 * register's device, created on first use): for a caller that has the next scan already.  The scan must stay untouched until the step
 * that takes it.  A filter queued earlier and never taken is collected and dropped.  The results do not depend on it. */
int pcr_frontend_prefetch(pcr_frontend* fe, const void* next_scan, size_t n, size_t stride_bytes, int on_device);
int pcr_frontend_finish(pcr_frontend* fe, size_t* n_submap);   /* collects a queued assembly */
int pcr_frontend_reset(pcr_frontend* fe);                      /* pcr_map_clear + the loop's own state; device memory kept */
/* mClosestKfIdx (MapManager.cpp:146), which Backend::addOdomFactor reads: one entry per key frame this front end has added since create or
 * reset, in order -- the index of the key frame whose squared distance step 6 found smallest (the lowest index on a tie), -1 for a key frame
 * added to an empty store.  Recording only: no step's result depends on it.  *n (may be NULL) = the entries there are; idx == NULL writes
 * the count alone; a capacity below the count fails and writes nothing else. */
int pcr_frontend_closest(const pcr_frontend* fe, int64_t* idx, size_t capacity, size_t* n);

/* ---- Key frames ranked by distance: the loop detector backend/DistContext.hpp declares (a kd-tree over key-frame positions) and leaves empty ----
 * For every query key frame q of [first, first + count) and every candidate i of [0, q - num_exclude_recent): the squared distance of their
 * positions, (dx*dx + dy*dy) + dz*dz in double, d = candidate - query, every operation rounded on its own (the order of pcr_frontend_step's
 * step 6).  A candidate counts when d2 <= radius*radius; of those the k best by (d2, i) ascending are kept -- the lower index wins a tie.
 * Row q - first of idx and d2 (count * k entries each) holds them in that order, the tail idx -1, d2 DBL_MAX.  k is 1..8.  A query or a
 * candidate with a coordinate that is not finite never matches.  A row depends on its query alone: the same bits whatever the window.
 * Fails, writing NOTHING, when k is out of range, radius is negative or not finite, num_exclude_recent < 0, first + count > n, or idx or d2
 * is NULL while count > 0; count == 0 returns 0.
 * pcr_kf_rank_near_host is the definition: host only, no GPU, positions xyz[3 n].  pcr_map_rank_near is the same over the positions of a
 * store's key frames (parent or view; the translations of the poses the store holds now), on the device: the positions of key frames
 * [0, first + count) go up once per call as three arrays of doubles, tiles of 16 queries meet the candidates in tiles of 256, every lane
 * keeps its k best in registers and a query's lanes are merged in a fixed order -- no atomics, the result depends on no schedule and equals
 * the host function's bit for bit.  Its failures report through pcr_map_last_error. */
int pcr_kf_rank_near_host(const double* xyz, size_t n, size_t first, size_t count, int num_exclude_recent, double radius, int k, int64_t* idx,
                          double* d2);
int pcr_map_rank_near(const pcr_map* m, size_t first, size_t count, int num_exclude_recent, double radius, int k, int64_t* idx, double* d2);

/* ---- The back end's key-frame and loop-closure loop -------------------------------------------------------------------------------------
 * Backend::optimHandler (backend/src/Backend.cpp:270-347) and LoopClosureManager::lcHandler (backend/src/LoopClosureManager.cpp:62-119)
 * strung together once, in the library, over handles that exist: a view of the store (lc_map_), a ScanContext database, a register with
 * initForLC's settings and a pose graph.  No thread, queue or condition variable: the caller decides when an event runs, as with
 * pcr_frontend.  The two events are pinned bit for bit to the same sequence of public calls made by a caller. */
typedef struct pcr_backend pcr_backend;
enum { PCR_BACKEND_SC_QUERY = 1, PCR_BACKEND_SC_RANK = 2, PCR_BACKEND_DISTANCE = 4 };      /* pcr_backend_params.detectors */
enum { PCR_VGICP = 0, PCR_GICP = 1 };                                                      /* pcr_backend_params.lc_method */
typedef struct pcr_backend_params {
    double grid_size;            /* 0.5  downSampleVoxelGridSize: saveKfs' in-place filter; <= 0: key frames are left as they are */
    double context_grid_size;    /* 0.5  backend.lc.contextDownSampleGridSize: contexts and the loop window */
    int32_t history_range;       /* 1    backend.lc.historySubmapRange */
    double fitness_threshold;    /* 0.3  backend.lc.fitnessThreshold */
    int32_t detectors;           /* bit 0 SC_QUERY (default, lcHandler's pcr_sc_query), bit 1 SC_RANK (pcr_sc_rank_stored k = 1 + dist_thres),
                                    bit 2 DISTANCE (pcr_map_rank_near, k = 1); 0: no loop is looked for */
    double dist_radius;          /* 5.0  DISTANCE: metres */
    int32_t dist_exclude_recent; /* DISTANCE: default -1 = sc.num_exclude_recent as pcr_backend_create finds it */
    int32_t lc_method;           /* PCR_VGICP (default, the reference's) or PCR_GICP */
    int32_t lc_between_refined;  /* 1 (default): the loop factor is old^-1 * refined pose; 0: the reference as written, old^-1 * cur (see below) */
    pcr_sc_params sc;
    pcr_graph_params graph;
} pcr_backend_params;
/* One candidate pair of pcr_backend_close_loops.  detector: the PCR_BACKEND_* bits of every detector that proposed the pair (it is verified
 * once).  converged, iterations, fitness: the registration of key frame cur against the window about old (pcr_fitness of the register);
 * a pair whose source or window is empty has converged 0, iterations 0, fitness DBL_MAX.  pose: the refined pose of cur. */
typedef struct pcr_backend_loop {
    int64_t cur, old;
    int32_t detector, converged, iterations, accepted;
    double fitness;
    double pose[16];
} pcr_backend_loop;
typedef struct pcr_backend_info {
    int64_t keyframes, contexts;     /* totals after the event: key frames in the graph, contexts in the database */
    int32_t keyframes_added;         /* add_keyframes: key frames this event took */
    int32_t candidates, accepted;    /* close_loops: pairs verified, pairs accepted */
    int32_t factors_added;           /* between factors this event added (odometry or loop) */
    int32_t optimized, pad_;         /* 1: pcr_graph_optimize and the pose write-back ran */
    pcr_graph_result graph;          /* ... and what it returned */
    double delta[16];                /* T2SE3(new_last * old_last^-1) of the newest key frame (graph.delta); the identity when nothing was optimised:
                                        what the caller applies to its global odometry and odom2map (Backend.cpp:321-346) */
    double seconds[9];               /* host time: contexts, downsample, factors, detect, window, scan2map, fitness, optimize, set_poses */
} pcr_backend_info;

void pcr_backend_default_params(pcr_backend_params* p);
/* Borrows `map` (a parent, not a view), which must outlive the back end; owns a view of it, a pcr_sc (params.sc), a register of lc_method
 * with initForLC's settings (100 iterations, translation epsilon 1e-6; gicp: correspondence distance 150) and a pcr_graph, all on the map's
 * device.  p == NULL: the defaults.  NULL on failure (pcr_backend_last_error(NULL)). */
pcr_backend* pcr_backend_create(pcr_map* map, const pcr_backend_params* p);
void pcr_backend_destroy(pcr_backend* be);
const char* pcr_backend_last_error(const pcr_backend* be);
/* The owned handles, for the interfaces that exist: a robust kernel, fixed poses, pcr_graph_save_g2o, the contexts, the register's stats. */
pcr_graph* pcr_backend_graph(pcr_backend* be);
pcr_sc* pcr_backend_sc(pcr_backend* be);
pcr_handle* pcr_backend_register(pcr_backend* be);
/* optimHandler's NewKFCome event for key frames [done, pcr_map_keyframes) (done: the key frames earlier events took), in the reference's order:
 *   1. pcr_sc_add_keyframes(map, done, count, context_grid_size): contexts from the RAW key frames, before saveKfs filters them;
 *   2. grid_size > 0: pcr_map_downsample_keyframes(map, done, grid_size) (saveKfs); with a save directory (pcr_backend_set_save_dir) the new key
 *      frames are written raw first;
 *   3. an empty graph: pcr_graph_add_prior on pose 0 at key frame 0's pose with pcr_graph_noise(PRIOR) (the factor may precede its pose);
 *   4. pcr_graph_add_poses of the new key frames' stored poses;
 *   5. per new key frame i > 0 pcr_graph_add_between_poses(closest[i - done], i, pcr_graph_noise(ODOM)); closest == NULL: from i - 1.
 *      closest (n_closest entries, at least count) is pcr_frontend_closest's tail for these key frames; an entry that is -1 for a key frame
 *      other than 0, at or beyond its own index, or out of range -- or an n_closest below count -- fails the call BEFORE anything changes;
 *   6. pcr_graph_optimize(params.graph);   7. pcr_map_set_poses_from_graph(map, graph, 0, all);   8. delta (info).
 * No new key frame: returns 0, nothing changes, delta is the identity. */
int pcr_backend_add_keyframes(pcr_backend* be, const int64_t* closest, size_t n_closest, pcr_backend_info* info);
/* lcHandler over contexts [lc_done, pcr_sc_size), then the LC event when a loop was accepted.  Candidates (cur, old) come from the enabled
 * detectors -- SC_QUERY: pcr_sc_query(cur); SC_RANK: pcr_sc_rank_stored(k = 1), kept when dist <= (float)sc.dist_thres; DISTANCE:
 * pcr_map_rank_near(view, dist_exclude_recent, dist_radius, k = 1) -- in ascending cur, within one cur in the detectors' bit order, a pair once.
 * Per candidate: pcr_map_update_window(view, old, history_range, context_grid_size); source = pcr_map_keyframe(cur) in HBM;
 * pcr_scan2map_submap from guess = pose(cur); pcr_fitness.  Accepted when it converged and fitness < fitness_threshold: pcr_graph_add_loop
 * (old, cur, Z, pcr_graph_noise(LOOP)).  Z = pose(old)^-1 * guess -- the inverse as [R^T, -(R^T t)], the product row by row as
 * ((a0 b0 + a1 b1) + a2 b2) (+ t), in double without contraction.  lc_between_refined = 0 gives the reference as written
 * (LoopClosureManager.cpp:97-107 registers into `guess` and then builds the factor from cur_pose, the UNREFINED pose): Z = X_old^-1 X_cur of
 * the current estimates (pcr_graph_add_between_poses + the robust mark), a factor that agrees with the estimate and corrects nothing.
 * Then, when a factor was added: pcr_graph_optimize, pcr_map_set_poses_from_graph(0, all), delta.  iSAM2's update counts (1, then 3 more
 * after a loop) are not reproduced: the graph is optimised to params.graph's own convergence.  The records stay readable through
 * pcr_backend_loops until the next pcr_backend_close_loops or reset. */
int pcr_backend_close_loops(pcr_backend* be, pcr_backend_info* info);
/* The records of the last pcr_backend_close_loops; *n (may be NULL) = how many there are; out == NULL writes the count alone; a capacity
 * below the count fails and writes nothing else. */
int pcr_backend_loops(const pcr_backend* be, pcr_backend_loop* out, size_t capacity, size_t* n);
/* The two events in order; either info may be NULL.  close_loops runs also when no key frame was new (it then finds no new context). */
int pcr_backend_step(pcr_backend* be, const int64_t* closest, size_t n_closest, pcr_backend_info* add_info, pcr_backend_info* loop_info);
/* Starts over: the graph, the contexts, the records and the counters are cleared, the store is left alone (device memory kept).
 * Failures follow pcr_frontend's rule: the inner call's message under the step's name, the state what the completed parts left, further
 * events refused until pcr_backend_reset. */
int pcr_backend_reset(pcr_backend* be);

/* ---- A session on disk: key-frame clouds, poses, graph and contexts ------------------------------------------------------------------------
 * The reference's saveMapDir: {i}.pcd, the RAW key frame i (MapManager::saveKfs, frontend/src/MapManager.cpp:203-213); tum.txt, one pose per
 * key frame (utils::file::writeAsTum in Backend::~Backend, common/utils/File.hpp:49-66, backend/src/Backend.cpp:349-358); fg.g2o, the factor
 * graph (myWriteG2o).  MapManager::MapManager() (MapManager.cpp:18-50) and Backend::Gtsam::loadFactorGraph (Backend.cpp:202-222) read it at
 * the next start.  No kernel of its own: a load is pcr_map_add_keyframe, pcr_sc_add_keyframes, pcr_map_downsample_keyframes and
 * pcr_graph_load_g2o in the back end's order.  DESIGN 4.19.
 *
 * The file formats, host only (no GPU is needed to call them).  Their failures leave a message in pcr_session_last_error (per thread). */
const char* pcr_session_last_error(void);
/* One line of writeAsTum into buf, NUL-terminated: "%.3f %.3f %.3f %.3f %.6f %.6f %.6f %.6f\n" of stamp, t, q.x, q.y, q.z, q.w; the
 * quaternion is Eigen::Quaternion(R)'s (the trace / largest-diagonal branches T2SE3 uses, NOT normalised); pose16 is column-major.  The
 * format is LOSSY: a translation comes back within 5e-4 m, a quaternion component within 5e-7.  precise != 0 writes every number as %.17g
 * instead: every double comes back as it was.  Nonzero when the stamp or the pose is not finite, or when capacity cannot hold the line
 * and its NUL (the message says how many bytes it takes; buf is left alone). */
int pcr_tum_format(double stamp, const double pose16[16], int precise, char* buf, size_t capacity);
/* One line as loadFromTum reads it (File.hpp:69-95): stamp, t.x t.y t.z, q.x q.y q.z q.w, separated by blanks; what follows the eighth
 * number is ignored.  pose = identity . translate(t) . rotate(q) with Eigen's toRotationMatrix of the quaternion AS READ, NOT normalised
 * (the products with the identity are not carried out: they could change the sign of a zero and nothing else): six digits give a rotation
 * that is orthonormal to about 1e-6 only, and a caller who wants more applies T2SE3.  PCR_TUM_OK: stamp (may be NULL) and pose16 are
 * written.  PCR_TUM_SKIP: the line is empty or blank and nothing is written (the reference pushes a pose built from uninitialised numbers
 * there).  PCR_TUM_ERROR: fewer than eight numbers; the message quotes the line. */
enum { PCR_TUM_OK = 0, PCR_TUM_ERROR = 1, PCR_TUM_SKIP = 2 };
int pcr_tum_parse(const char* line, double* stamp, double pose16[16]);
/* pcp::savePCDFile (binary: pcl::io::savePCDFileBinary's "x y z intensity" F 4) and pcp::loadPCDFile over host memory of n points,
 * stride_bytes apart (a multiple of 4, >= 12).  The intensity is float 3 of a 16-byte point, float 4 of a point of 20 bytes or more
 * (pcl::PointXYZI: float 3 is then written as 1 on a read and the floats behind the intensity as 0) and absent from a 12-byte point (0 in
 * the file).  n = 0 writes a valid file with POINTS 0, which reads back as 0 points.  Non-finite values travel as their bytes.
 * read: *n is the file's point count whenever the header could be read; a capacity below it fails and writes nothing else (out == NULL
 * with capacity 0: the count alone).  The reader takes every PCD the mirror's takes: ascii, binary, binary_compressed, any field order. */
int pcr_pcd_write(const char* path, const void* pts, size_t n, size_t stride_bytes);
int pcr_pcd_read(const char* path, void* out, size_t capacity_points, size_t stride_bytes, size_t* n);

/* {dir}/{i}.pcd for key frames [first, n) as the store holds them NOW (after pcr_map_downsample_keyframes: the filtered clouds; the raw
 * ones can only be written before it, see pcr_backend_set_save_dir) and {dir}/tum.txt, rewritten, for ALL n key frames.  stamps: n
 * entries, or NULL for stamp i = i.  A queued assembly is collected first.  Parent or view; the directory must exist; first > n is an
 * error.  The first failure names the file (pcr_map_last_error) and leaves earlier files as written. */
int pcr_map_save(const pcr_map* m, const char* dir, size_t first, const double* stamps, int precise);
/* The loading constructor (MapManager.cpp:33-49) into a store WITHOUT key frames (else refused, nothing changed): line i of {dir}/tum.txt
 * (blank lines do not count) gives the pose of {dir}/{i}.pcd, added by pcr_map_add_keyframe in the store's point layout (16 bytes when it
 * never held a key frame); grid_size > 0: then pcr_map_downsample_keyframes(m, 0, grid_size) (:46).  The poses are NOT normalised.
 * stamps (may be NULL) gets the first `capacity` stamps; *n_loaded (may be NULL) the number of key frames.  Every file is read and checked
 * before the store changes: a missing or unreadable PCD or a bad line fails with the store still empty and a message that names the file
 * or the line (1-based).  A missing tum.txt returns 0 with *n_loaded = 0: the reference warns and starts fresh. */
int pcr_map_load(pcr_map* m, const char* dir, double grid_size, double* stamps, size_t capacity, size_t* n_loaded);

/* saveMapDir of the back end.  NULL or "": off (the default), every call does what it did.  Set: step 2 of pcr_backend_add_keyframes
 * writes {dir}/{i}.pcd of each new key frame RAW, before the in-place filter (saveKfs' order: the filter destroys the raw cloud, so this
 * is the one moment it can be saved); a failure there is the event's failure under the step name "save". */
int pcr_backend_set_save_dir(pcr_backend* be, const char* dir);
/* What ~Backend does: {dir}/tum.txt of all key frames of the store (pcr_map_save's writer; stamps: one per key frame or NULL) and
 * {dir}/fg.g2o (pcr_graph_save_g2o: no priors, robust marks or switches; FIX records and switched-off factors as it writes them).
 * Refused without a save directory. */
int pcr_backend_save(pcr_backend* be, const double* stamps, int precise);
/* A session back into a freshly created or reset back end over an EMPTY store, in the back end's own order:
 *   1. pcr_map_load(map, dir, grid_size <= 0): the raw key frames;
 *   2. pcr_sc_add_keyframes(map, 0, n, context_grid_size): the contexts from the raw clouds.  (The reference builds none for loaded key
 *      frames -- addContext starts at mKFNums -- so a second session there never closes a loop onto the first; here it can.)
 *   3. params.grid_size > 0: pcr_map_downsample_keyframes(map, 0, grid_size);
 *   4. pcr_graph_load_g2o(graph, dir/fg.g2o).
 * Then the counters stand behind the loaded key frames: the next pcr_backend_add_keyframes takes the key frames added after the load,
 * pcr_backend_close_loops their contexts as queries with every loaded key frame as a candidate.  The store's poses are tum.txt's; the
 * graph's are its own vertices until the next optimisation writes them back.  info (may be NULL): keyframes, contexts, keyframes_added,
 * seconds[contexts, downsample, factors = the graph's load]; pcr_backend_load_seconds has the whole split.  stamps / capacity as
 * pcr_map_load.  Refused BEFORE anything changes: key frames in the store or poses in the graph or contexts in the database; no fg.g2o
 * (without the graph the first component has no prior: pcr_map_load is the map-only load, and the message says so); a fg.g2o that does
 * not load or whose vertex count differs from tum.txt's key-frame count; a bad line or PCD.  A failure after that (a HIP error) leaves
 * the back end failed until pcr_backend_reset, as with the events. */
int pcr_backend_load(pcr_backend* be, const char* dir, double* stamps, size_t capacity, pcr_backend_info* info);
/* Host time of the last pcr_backend_load: reading the files, uploading the key frames, contexts, in-place filter, graph. */
int pcr_backend_load_seconds(const pcr_backend* be, double seconds[5]);

#ifdef __cplusplus
}
#endif
#endif /* PCR_HIP_H */
