// pcr_internal.h -- shared host/device declarations of libpcr_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>

#include <stdlib.h>

#include "../../include/pcr_hip.h"
#include "grid_plan.h"
#include "sparse_walk.h"

namespace pcr {

// ---------------------------------------------------------------------------
// Uniform-grid spatial index over the target cloud ("voxel tiles").
//
// Replaces the reference's per-call nanoflann kd-tree (LoamRegister.cpp:110;
// nanoflann.hpp:1542-1564).  Cell edge = the k-NN gate radius (1 m for the
// reference constants), so every neighbour that can pass the gate
// lies in the 3x3x3 block around the query's cell.  Points are counting-sorted by
// linear cell key (x fastest), so the three x-adjacent cells of one (y,z) row
// are ONE contiguous run of float4s: a query reads 9 runs.
// ---------------------------------------------------------------------------
struct GridHeader {
    double origin[3];        // lower corner of cell (0,0,0) = org * cell
    double org[3];           // integer-valued: cell (i,j,k) spans [(org+i)*cell, (org+i+1)*cell)
    double cell;             // edge length (a power of two >= gate radius: x/cell is exact)
    double inv_cell;
    int32_t dims[3];         // cells per axis, including 2 pad cells on every side
    uint32_t n_points;       // points the build that wrote the header was given (the number INDEXED -- finite, inside the box -- is cell_start[n_cells])
    uint64_t n_cells;        // dims[0]*dims[1]*dims[2]
    int32_t overflow;        // n_cells + 1 exceeds the allocated cell table
    int32_t empty;           // no finite point
    double shift;            // lattice offset in cells: cell index = floor(x / cell - shift) - org (0.5 for the VGICP voxel lattice)
    // pcl::VoxelGrid lattice (voxel_filter.hip): cell index = (int)(floorf(x * inv_leaf_f) - (float)min_b), all in float,
    // dims = max_b - min_b + 1 without pad cells.  pcl_mode = 0 everywhere else.
    int32_t pcl_mode;
    float inv_leaf_f;
    int32_t min_b[3];
    int32_t too_fine;        // pcl_mode: more than INT_MAX voxels ("Leaf size is too small", voxel_grid.hpp)
    float sum_sq;            // sum over the cells of count^2 (written by the scan of the atomic build path): sum_sq / points =
                             // occupancy of the cell a point lives in, averaged over the points -- the density estimate behind the
                             // choice of a search cell.  The tiled build path accumulates the same sum exactly in sum_sq_u.
    int32_t clamped;         // the box was cut to a region of interest (ClampBox): points outside it are not indexed
    int32_t cut_mask;        // clamped: bit d = the lower face of axis d was cut (target points lie beyond it), bit 3 + d = the upper
    unsigned long long sum_sq_u;
    int32_t stale;           // the header was reused from the previous build (bounding-box hint) and a point of the new cloud lies
    int32_t pad2_;           // outside its box: the index is incomplete, the caller rebuilds with a fresh box
};
__host__ __device__ inline double grid_sum_sq(const GridHeader& h) { return h.sum_sq_u ? (double)h.sum_sq_u : (double)h.sum_sq; }

// Region of interest for an index whose full bounding box cannot be tabulated (a far outlier in the cloud): see loam_host.hip
struct ClampBox { double lo[3], hi[3]; int32_t use, pad_; };

struct HeaderTwin { GridHeader* hdr; GridHeader* mirror; uint64_t capacity; double cell; };      // grid_bbox_header_kernel: a second header from the same box

struct GridView {            // what kernels need to query the index
    const GridHeader* hdr;
    const float4* pts;       // sorted by cell; .w = original index (uint bits)
    const uint32_t* cell_start;  // n_cells + 1 entries
};

static constexpr int kPad = 2;           // pad cells per side (see grid_index.hip)
// progress word of the device-resident optimisers (NdtOut / VgOut): call number * kProgressWindow + passes consumed.  The pass budget
// of a call ((ndt_max_iters + 3) * 13 + 5, vgicp_max_iters * lm_inner + 3) must stay inside the window: checked by pace_passes (handle.h).
static constexpr double kProgressWindow = 1048576.0;

struct Pose16 { double m[16]; };

// ---------------------------------------------------------------------------
// LOAM Gauss-Newton state carried between launches (device memory).
// ---------------------------------------------------------------------------
struct LoamState {
    double pose[16];     // column-major map<-lidar
    int32_t done;        // 1: loop finished (converged, too few points, or error)
    int32_t converged;   // isConverge (PointCloudRegister.hpp:15)
    int32_t iters_run;   // linearisations whose result was consumed
    int32_t fail;        // 1: fewer than 6 accepted points (LoamRegister.cpp:173-176)
                         // 2: sharded call, some rank could not index its tile (kSlotRankFail)
                         // 3: a query came within one cell of a cut face of a clamped index (kSlotEscapes): the call is redone
};

static constexpr int kAccum = 32;        // 21 JtJ (upper) + 6 JtE + 1 count, padded; [28], [29] search statistics and
static constexpr int kSlotRankFail = 30; //   sharded: > 0 when a rank's index is unusable (summed over the ranks by the exchange)
static constexpr int kSlotEscapes = 31;  //   queries that left the region a clamped index covers
static constexpr int kMaxPartials = 512; // linearisation blocks
static constexpr int kTimelineSlots = 24; // s_memrealtime stamps per block and launch (pcr_get_timeline)

struct LoamConsts {
    double knn_max_sq, plane_thresh, point_thresh, pos_conv, rot_conv;
    int32_t iters, early_exit;
};

struct LoamResult {          // written by the finalize launch into host-mapped memory
    double pose[16];         // after T2SE3
    int32_t converged, iters_run, fail, grid_overflow, grid_empty, pad;
    uint64_t grid_cells;     // cells the target needs (to grow the table on overflow)
    int32_t grid_stale;
    int32_t progress;        // (launch whose prologue has run) << 1 | the loop has ended: written by every launch's prologue, read by a host that queues launches a few ahead (run_loam, early exit)
};

struct LoamTrace {           // per consumed linearisation
    double JtJ[36];
    double JtE[6];
    double x[6];
    int64_t n;
    int64_t cache_hits, searches;   // queries served by the neighbour cache / by a full search in that linearisation
};

// The LOAM neighbour cache in memory (loam.hip reads and writes it, fill_loam_args sizes it): the entries of 64 consecutive scan
// points -- one wave's -- form one tile, ordered [field][lane], so that every 16-byte field of a wave is 1 KB of contiguous memory.
static constexpr int kCacheFields = 12;                                              // 16-byte fields of an entry (NnCacheEntry)
static constexpr size_t kCacheTileBytes = (size_t)kCacheFields * 64 * 16;
// (one spare tile behind the last: where the waves of a block without a single scan point aim their fetch)
static inline size_t loam_cache_bytes(size_t n_src) { return ((n_src + 63) / 64 + 1) * kCacheTileBytes; }

struct LoamArgs {
    const float* src;        // scan points, stride in floats
    uint32_t n_src;
    uint32_t src_stride;
    GridView grid;
    LoamConsts c;
    double init_pose[16];    // initial guess, consumed by launch 0
    LoamState* state;        // [2], ping-pong by launch parity
    double* partials;        // [2][kMaxPartials][kAccum]
    const double* reduced;   // non-null: partial sums already reduced (and all-reduced) into kAccum doubles
    uint32_t n_partials;     // blocks of the linearisation grid
    LoamTrace* trace;        // [iters] or null
    LoamResult* result;      // final pose (after T2SE3) and flags
    // optional per-point outputs (tests): null in production
    int8_t* dbg_status;
    double* dbg_rows;
    int32_t* dbg_nn;
    // optional query tile (multi-GPU): process only queries inside [lo,hi)
    float4* nn_cache;        // [tiles][kCacheFields][64] neighbours of the previous iteration (loam.hip: entry_field), or null
    int32_t use_tile;
    double tile_lo[3], tile_hi[3];
    int32_t coresident;      // pcr_params.loam_coresident = 1: the two-waves-per-SIMD variant of the iterate kernel (loam.hip)
    int32_t rank_fail;       // sharded: this rank has no usable index (its grid view is a dummy marked overflow); told to the others
    // profiling aid (pcr_params.record_timeline = 1): [launch][block][kTimelineSlots] s_memrealtime stamps (100 MHz) taken by thread 0
    unsigned long long* timeline;
};

// host-side launchers (grid_index.hip / loam.hip)
// A device allocation that frees itself with its owner; not copyable, so nothing else frees it too.  GridIndex and CovScratch, made
// of these, are freed and kept from copies the same way.
struct DeviceBuf {
    void* p = nullptr;
    size_t cap = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { release(); }
    hipError_t reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// A build that indexes only the points inside a region (pcr_scan2map of NDT: voxel Gaussians depend on a voxel's own points alone, so
// a lattice that holds nothing outside the region the scan can reach serves that scan as the full one would).  Possible only when the
// build reuses the header and the tile layout of a previous FULL build (the lattice the mask is laid over must be known before the
// points are binned, and the room of every tile is the full cloud's): build() then calls enqueue_mask -- which queues the marking of the
// region on the build's stream and fills mask / mshift -- and sets `applied`; otherwise it builds in full and leaves `applied` false.
// What the tile pass of a FILTERED build does for NDT while a tile's cell counts are still in LDS (grid_index.hip: grid_tile_kernel<.., kTail>):
// the cells inside the mask with at least min_points points are appended to `list` (one atomic on `count` per tile), the slot of every cell is
// written -- 0 inside the mask, kNdtUnprepared outside -- and `count_next` is cleared: what ndt_candidates_kernel does in a launch of its own
// by reading the finished table again (ndt.hip).
static constexpr uint32_t kNdtUnprepared = 0xffffffffu;      // slot of a cell the target was not prepared for (ndt.hip)
struct TileTail {
    uint32_t* vox_slot; uint32_t* list; uint32_t* count; uint32_t* count_next;
    int32_t min_points; uint32_t capacity;
    const uint8_t* mask; int32_t mshift;      // (filled by build() from the filter's mask)
};
struct BuildFilter {
    std::function<hipError_t()> enqueue_mask;
    const uint8_t* mask = nullptr;      // one byte per macro cell of the lattice (RoiView::mask)
    int mshift = 0;
    bool applied = false;
    bool want_tail = false;             // `tail` is filled in: the tile pass may list NDT's voxel cells
    TileTail tail = {};
    bool tail_applied = false;          // ... and did (only together with `applied`, on the dense tile kernel)
};

// The hints a build leaves for the next one, and the switches its owner sets, are the base (grid_plan.h: BuildHints): build() reserves, plans
// (plan_build: a pure host function), enqueues what the plan says and commits the hints (commit_build).
struct GridIndex : BuildHints {
    DeviceBuf sorted, cell_count, cell_start, block_sums, bbox_partials, header, keys, ranks, ticket;
    DeviceBuf kept;                             // region-only builds: the points of the region as (x, y, z, original index), listed by grid_keep_kernel for the bin pass
    DeviceBuf tiled, bin_count, bin_start, tile_sq;      // tiled build path: points grouped by tile, points per tile, first point of every tile, sum of count^2 per tile
    DeviceBuf layout[2];                        // the layout hint's two buffers, alternating (BuildHints::lay_idx)
    // A build WITHOUT hints computes the bounding box itself; then (grid_bbox_header_kernel)
    GridHeader* header_mirror = nullptr;        //   the header is also written to this host-mapped address (no copy queued behind the build): `mirrored` says so
    GridIndex* twin = nullptr;                  //   and `twin`, an index the caller builds NEXT over the same cloud with cell twin_cell, gets its header from the
    double twin_cell = 0.0;                     //   same pass (its build() then launches no box kernel)
    hipError_t ensure_tables(hipStream_t s, std::string* err);
    void confirm() { hint_ok = valid && tiled_shift >= 0; }
    size_t n_points = 0;
    size_t reserve_points = 0;  // build() sizes its point-sized buffers for at least that many points (a caller whose clouds grow: every growth is an allocation and a free, device-wide stops)
    bool valid = false;
    BuildPlan last_plan;        // what the last build() enqueued (completed with the answer of the filter's mask callback): for checks and statistics, read by no decision
    GridView view() const {
        return GridView{header.as<GridHeader>(), sorted.as<float4>(), cell_start.as<uint32_t>()};
    }
    // Enqueue the build of the index over n points (device pointer, stride in floats).
    // No host synchronisation unless the cell table must grow.  cell = grid edge.
    hipError_t build(const float* d_pts, size_t n, size_t stride_floats, double cell, hipStream_t s,
                     std::string* err, double shift = 0.0, int pcl_mode = 0, const ClampBox* clamp = nullptr, bool allow_hint = false,
                     BuildFilter* filter = nullptr);
    // build()'s third step: what the plan says, onto the stream (it completes the plan with the answer of the filter's mask callback)
    hipError_t enqueue_build(BuildPlan& p, BuildRequest& rq, size_t n_res, const ClampBox& cb, hipStream_t s, std::string* err, BuildFilter* filter);
    // Make room for `need_cells` cells (+1 start) after the device reported overflow.
    hipError_t grow_cells(uint64_t need_cells, std::string* err);
    // header.sum_sq_u <- sum over the cells of count^2 (enqueued; VGICP reads it back with the header)
    hipError_t enqueue_density(hipStream_t s);
    void release();
};

// ---------------------------------------------------------------------------
// VGICP (vgicp.hip)
// ---------------------------------------------------------------------------
struct VgicpVoxel {          // fast_vgicp_voxel.hpp:57-122 (GaussianVoxel, finalized: ADDITIVE or MULTIPLICATIVE)
    double mean[3];
    double cov[6];           // xx xy xz yy yz zz
    double w;                // sqrt(num_points)
    uint32_t n, pad;
};

// Region of interest of a target that is prepared for ONE scan (pcr_scan2map: the reference rebuilds its target structures for every
// call -- fast_vgicp_impl.hpp:66-67, ndt_omp.h:276-283 -- but a scan can only ever look up the voxels near where its points land).
// The lattice of the target index is grouped into macro cells of 2^mshift cells per axis (about 2 m); the macro cells that hold a scan
// point at the initial pose are marked, every mark is spread over the macro cells within base + 0.05 x (distance from the sensor) metres
// -- a translation of `base`, a rotation of 0.05 rad (grid_index.hip: roi_*) -- and only voxels inside marked macro cells are prepared (per-point covariances + voxel Gaussians for VGICP, voxel Gaussians for NDT).  Every lookup of the
// optimiser checks the cell it hits: an occupied cell OUTSIDE the region is counted in *escapes, and the host then prepares the whole
// target and repeats the call -- so the result is the full preparation's whenever the call succeeds (a pose that moves the scan by
// more than the margin is rare and merely costs the repeat).
struct RoiView {
    const GridHeader* lat;       // the lattice (header of the target index); macro dims = ceil(dims / 2^mshift)
    const uint8_t* mask;         // one byte per macro cell, != 0: prepared.  nullptr: no region -- everything is prepared
    uint32_t* escapes;
    int32_t mshift;
    int32_t filtered;            // the index itself holds the region's points only (BuildFilter): NDT then treats EVERY cell outside the mask as unprepared
    uint32_t* count;             // profiling passes only (pcr_set_profile >= 2), else nullptr: [0] += target points whose covariance was computed, [16] += voxels built
};
__host__ __device__ inline uint32_t roi_macro(const GridHeader& h, int mshift, int cx, int cy, int cz) {      // cell (cx, cy, cz) inside the lattice
    const uint32_t m0 = ((uint32_t)h.dims[0] + (1u << mshift) - 1u) >> mshift, m1 = ((uint32_t)h.dims[1] + (1u << mshift) - 1u) >> mshift;
    return (((uint32_t)cz >> mshift) * m1 + ((uint32_t)cy >> mshift)) * m0 + ((uint32_t)cx >> mshift);
}
__host__ __device__ inline bool roi_mask_holds_cell(const GridHeader& h, const uint8_t* mask, int mshift, uint32_t key) {      // linear cell key
    const uint32_t d0 = (uint32_t)h.dims[0], d1 = (uint32_t)h.dims[1], row = key / d0, cz = row / d1;
    return mask[roi_macro(h, mshift, (int)(key - row * d0), (int)(row - cz * d1), (int)cz)] != 0;
}
#ifdef __HIPCC__
// is the voxel that the point (x, y, z) belongs to inside the prepared region?  (lat: the voxel lattice's header)
__device__ __forceinline__ bool roi_holds_point(const RoiView& roi, const GridHeader& lat, double x, double y, double z) {
    const double fx = floor(x / lat.cell - lat.shift) - lat.org[0], fy = floor(y / lat.cell - lat.shift) - lat.org[1], fz = floor(z / lat.cell - lat.shift) - lat.org[2];
    if (!(fx >= 0.0 && fx < (double)lat.dims[0] && fy >= 0.0 && fy < (double)lat.dims[1] && fz >= 0.0 && fz < (double)lat.dims[2])) return false;
    return roi.mask[roi_macro(lat, roi.mshift, (int)fx, (int)fy, (int)fz)] != 0;
}
#endif
// A few hundred words a kernel stores on the side for a later launch on its stream: the initial state of NDT's device-resident optimiser rides
// on the first launch of its call (the region's mark pass).  A launch of its own cost ~5 us -- a kernel reads its argument block over PCIe --
// and ~2 us of gap, on a stream where nothing else could run meanwhile.
struct BlobStore { uint32_t* dst; uint32_t* zero; uint32_t n; uint32_t pad; uint32_t w[416]; };
hipError_t roi_launch(const GridIndex& lattice, const float* d_src, size_t n_src, size_t stride_floats, const Pose16& T, int mshift,
                      uint8_t* d_mark, uint8_t* d_mark_next, uint8_t* d_tmp, uint8_t* d_mask, double base_m, double per_m, hipStream_t s,
                      const BlobStore* blob = nullptr);

struct VgicpArgs {
    const float* src; uint32_t n_src, src_stride;
    const double* src_cov6;      // per source point, original order
    const GridHeader* hdr;       // target index header (voxel lattice = index grid shifted by half a cell)
    const uint32_t* cell_start;  // of the target index: voxel = cell, stored at the position of the cell's first point
    const VgicpVoxel* vox;
    uint32_t* corr_slot;         // DIRECT1: [n_src] voxel slot + 1 of the correspondence, 0 = none.  DIRECT7 / DIRECT27 (K = 7 / 27 table entries):
                                 //   [K + 1][n_src] -- row k the slot + 1 of the pair with table entry k, row K the point's presence bits (bit k)
    double* corr_M;              // DIRECT1: [n_src][6] Mahalanobis matrix of the correspondence.  DIRECT7 / DIRECT27: not used (vgicp.hip: storage)
    double* corr_T;              // DIRECT7 / DIRECT27: [16] the pose of the linearisation that wrote corr_slot: compute_error derives every pair's M from it
    uint32_t* corr_slot_next;    // the same three for the linearisation an LM trial pass computes ahead (vgicp_launch_error)
    double* corr_M_next;
    double* corr_T_next;
    double* partials;            // [blocks][32]
    int32_t use_tile;            // sharded target: only source points whose transformed position lies in [tile_lo, tile_hi)
    int32_t search;              // pcr_params.vgicp_search (PCR_VGICP_DIRECT*): read by the HOST launchers only, which pick the kernel instantiation by it
    double tile_lo[3], tile_hi[3];
    uint32_t* escapes;           // target index cut to the bulk of the cloud (header.clamped): count of source points that land within
    int32_t guard_cells, pad2_;  //   guard_cells voxels of a face with target points beyond it (their voxels' covariances may lack neighbours); else NULL
    RoiView roi;                 // mask == nullptr: the whole target is prepared
};
// the arguments of a pass whose state has `parity` set: the two pairs of correspondence buffers change places (VgCtl::parity)
__host__ __device__ inline VgicpArgs swapped(VgicpArgs a, int parity) {
    if (parity) {
        uint32_t* const s = a.corr_slot; a.corr_slot = a.corr_slot_next; a.corr_slot_next = s;
        double* const m = a.corr_M; a.corr_M = a.corr_M_next; a.corr_M_next = m;
        double* const t = a.corr_T; a.corr_T = a.corr_T_next; a.corr_T_next = t;
    }
    return a;
}

// Halo check of a sharded target (pcr_set_shard): for every point inside [chk_lo, chk_hi) the 20th neighbour must be nearer
// than the faces of [ext_lo, ext_hi) -- the region the rank's cloud is complete in; *violations counts the others.
struct CovCheck { double chk_lo[3], chk_hi[3], ext_lo[3], ext_hi[3]; uint32_t* violations; };
// Work memory of the two-class covariance search of a scan-sized cloud (cov_search.hip): neighbour lists [20][n], the queue of the queries
// the lane-per-query kernel hands to the wave-per-query one (+ the bound each brings along), its counter.  One per stream that runs it.
struct CovScratch {
    DeviceBuf nbr, queue, seed, count;
    // a map-sized target prepared for one scan (vgicp.hip: vgicp_region_list_kernel): the sorted positions of the region's points, and two counters
    // used alternately (each call leaves the other one cleared for the next)
    DeviceBuf region_list, region_count;
    int region_idx = 0;
    hipError_t reserve(size_t n);
    hipError_t reserve_region(size_t n, hipStream_t s);
    void release();
};
// ev (optional, profiling passes): 6 events = begin / end of the three kernels
hipError_t cov_search_launch(const GridIndex& grid, const GridIndex* coarse1, const GridIndex* coarse2, const float* d_orig, size_t stride_floats,
                             size_t n, double* d_cov6, hipStream_t s, const CovCheck* check, const RoiView* roi, CovScratch& sc, int reg, hipEvent_t* ev = nullptr);
// scratch: scan-sized clouds (n <= 300 000) go through cov_search.hip when given one
// reg: pcr_params.vgicp_regularization (PCR_REG_*, validated by the caller); mode: pcr_params.vgicp_voxel_mode (PCR_VOXEL_*): no defaults, a caller names them
hipError_t vgicp_launch_cov(const GridIndex& grid, const GridIndex* coarse1, const GridIndex* coarse2, const float* d_orig, size_t stride_floats,
                            size_t n, double* d_cov6, hipStream_t s, int reg, const CovCheck* check = nullptr, const RoiView* roi = nullptr,
                            CovScratch* scratch = nullptr, hipEvent_t* ev = nullptr);
hipError_t vgicp_launch_voxels(const GridIndex& grid, const double* d_cov6, VgicpVoxel* d_vox, hipStream_t s, int reg, int mode, const RoiView* roi = nullptr);
// (seq: written last into d_out32[31] / d_out48[47], host-mapped: the completion word the host spins on)
hipError_t vgicp_launch_linearize(const VgicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq = 0.0);
// device-resident Levenberg-Marquardt loop (vgicp_opt.h): state in HBM, result in host-mapped memory
struct VgCtl;
struct VgOut;
hipError_t vgicp_launch_ctl_init(VgCtl* d_ctl2, const Pose16& guess, int max_iters, int lm_inner, double lm_init_scale, double rot_eps, double trans_eps, hipStream_t s,
                                 uint32_t* d_roi_escapes = nullptr);
struct PeerComm;
hipError_t vgicp_launch_pass_pro(const VgicpArgs& a, VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, hipStream_t s, double seq, int index,
                                 const PeerComm* pc = nullptr, double xseq = 0.0, double* d_reduced = nullptr);
// out32[28] = compute_error(T); out32[0..27] = the linearisation at T (correspondences into a.corr_*_next)
hipError_t vgicp_launch_error(const VgicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq = 0.0);
// out32[0] = sum of the squared 1-NN distances <= max_range, [1] = their number, [2] = (tile given) source points whose nearest
// neighbour could lie outside [ext_lo, ext_hi)
struct FitTile { int32_t use, pad_; double lo[3], hi[3], ext_lo[3], ext_hi[3]; };
hipError_t fitness_launch(const GridIndex& grid, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16], double max_range,
                          double* d_partials, double* d_out32, hipStream_t s, double seq = 0.0, const FitTile* tile = nullptr);
uint32_t vgicp_blocks(uint32_t n_src);
// the fold of a pass's [block][32] rows into d_out32 (vgicp.hip: sum_partials_kernel), `seq` written last into d_out32[31]
hipError_t sum_partials_launch(const double* d_partials, uint32_t nblocks, double* d_out32, hipStream_t s, double seq = 0.0);
// the same score and the batched one (fitness_batch_launch below) on the sparse target index (sparse_fitness.hip): the same launch shape, the same
// order of summation and the same outputs, out32[2] / RelocSum::viol always 0 -- the index holds every finite point of the target
struct RelocPart;
struct RelocSum;
hipError_t sparse_fitness_launch(const sw::View& v, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16], double max_range,
                                 double* d_partials, double* d_out32, hipStream_t s, double seq = 0.0);
hipError_t sparse_fitness_batch_launch(const sw::View& v, const float* d_src, size_t n_src, size_t stride_floats, size_t m, const float* d_poses,
                                       size_t n_poses, double max_sq, RelocPart* d_part, RelocSum* d_out, hipStream_t s);

// ---------------------------------------------------------------------------
// GICP (gicp.hip): fast_gicp::FastGICP, correspondences by exact nearest neighbour
// ---------------------------------------------------------------------------
struct GicpArgs {
    const float* src; uint32_t n_src, src_stride;
    const double* src_cov6;      // per source point, original order
    GridView grid;               // index of every finite target point
    const float* tgt;            // the target's points as the caller gave them (b_j is read at the original index j)
    uint32_t tgt_stride, pad_;
    const double* tgt_cov6;      // per target point, original order
    uint32_t* corr;              // [n_src] original index of the correspondence, 0xffffffff = none
    double* corr_M;              // [n_src][6] Mahalanobis matrix of the correspondence
    uint32_t* corr_next;         // the same two for the linearisation an LM trial pass computes ahead (gicp_launch_error)
    double* corr_M_next;
    double* partials;            // [blocks][32]
    float thr2, pad2_;           // the gate: a correspondence needs d2 < thr2 (float; +inf by default)
    float* d2_out;               // introspection (pcr_gicp_linearize): [n_src] float squared distance of the correspondence, +inf for none; else NULL
};
__host__ __device__ inline GicpArgs swapped(GicpArgs a, int parity) {      // (as VgicpArgs')
    if (parity) { uint32_t* const s = a.corr; a.corr = a.corr_next; a.corr_next = s; double* const m = a.corr_M; a.corr_M = a.corr_M_next; a.corr_M_next = m; }
    return a;
}
hipError_t gicp_launch_linearize(const GicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq = 0.0);
// out32[28] = compute_error(T) on a.corr / a.corr_M; out32[0..27] = the linearisation at T (correspondences into a.corr_*next)
hipError_t gicp_launch_error(const GicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq = 0.0);
hipError_t gicp_launch_pass_pro(const GicpArgs& a, VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, hipStream_t s, double seq, int index);
// ---------------------------------------------------------------------------
// LIORF (liorf.hip): LioScan2map of the reference's test/comp/liorf_scan2map.cpp; the optimiser's state machine is liorf_opt.h
// ---------------------------------------------------------------------------
struct LiorfCtl;
struct LiorfOut;
struct LiorfConsts {
    double knn_max_sq, plane_thresh, point_thresh, rot_conv_deg, trans_conv_cm, degenerate_eig;
    int32_t iters, min_rows, file_row, pad_;
};

struct LiorfArgs {
    const float* src; uint32_t n_src, src_stride;
    GridView grid;               // index of every finite target point
    const float* tgt;            // the target's points as the caller gave them (a neighbour is read at its original index)
    uint32_t tgt_stride, pad_;
    LiorfConsts c;
    float six0[6];               // the initial six numbers, consumed by launch 0
    double* partials;            // [blocks][32]: 21 AtA (upper triangle, row by row), 6 AtB, [27] the rows
    // introspection (pcr_liorf_linearize), else NULL: kept[n_src], coeff4[n_src][4]
    uint8_t* kept_out;
    float* coeff_out;
    LoamTrace* trace;            // [iters] per consumed linearisation (pcr_params.record_trace: JtJ = AtA, JtE = AtB, as rounded to float), or NULL
};
hipError_t liorf_launch_pass(const LiorfArgs& a, LiorfCtl* d_ctl2, double* d_rows2, LiorfOut* d_out, hipStream_t s, double seq, int index);
// one linearisation at a.six0 and nothing else: the launch above on a state that ends after it, then the fold of its rows into d_out32
// ([0..27] as the partials, `seq` into [31]); the float 4x4 it used is left in d_ctl2[0]
hipError_t liorf_launch_linearize(const LiorfArgs& a, LiorfCtl* d_ctl2, double* d_rows2, LiorfOut* d_out, double* d_out32, hipStream_t s, double seq);
uint32_t liorf_blocks(uint32_t n_src);

// pcr_fitness_batch (reloc.hip): the gated score of n_poses poses (d_poses: 16 floats each, column-major) of the subset i_j = floor(j n_src / m),
// j < m, of the source.  d_part: n_poses x ceil(m / 256) partials; d_out[h]: the sum of the counted squared distances, their number, and the
// number of points whose nearest target point may lie beyond a cut face of the index (fitness_kernel's out32[0..2])
struct RelocPart { double sum; uint32_t cnt, viol; };
// the device a ScanContext database lives on (scancontext.hip)
int sc_device(const pcr_sc* sc);
// the device a key-frame store, or a view of one, lives on (submap.hip)
int map_device(const pcr_map* m);
// (submap.hip, for kf_rank.hip) sets pcr_map_last_error's message and returns 1; a device buffer of at least `bytes` that belongs to this
// pcr_map object (contents not kept between calls), NULL when it cannot grow
int map_set_error(const pcr_map* m, const std::string& s);
void* map_scratch(const pcr_map* m, size_t bytes);
// the device a pose graph lives on, PCR_GRAPH_HOST (-2) for a graph without one (graph_host.hip)
int graph_device(const pcr_graph* g);
struct RelocSum { double sum; unsigned long long cnt, viol, pad_; };
hipError_t fitness_batch_launch(const GridIndex& grid, const float* d_src, size_t n_src, size_t stride_floats, size_t m, const float* d_poses,
                                size_t n_poses, double max_sq, RelocPart* d_part, RelocSum* d_out, hipStream_t s);
// its second launch alone: d_part[pose][chunk] folded in chunk order into d_out[pose]
hipError_t fitness_batch_reduce_launch(const RelocPart* d_part, size_t n_poses, uint32_t chunks, RelocSum* d_out, hipStream_t s);

// pcr_knn / pcr_radius_search (knn_query.hip): exact queries in f64 on an index that holds every point of its cloud (any lattice kind; the
// caller has checked the header: not overflowing, stale or cut).  d_idx / d_d2 of the k-NN: n_q x k, ascending by (d2, index), tails -1 / +inf.
// The radius search in passes: the counts and their exclusive scan (d_offsets: n_q + 1), the fill of every query's segment, its sort by
// (d2, index) from one pair of arrays into another.
hipError_t knn_query_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, int k, int64_t* d_idx, double* d_d2, hipStream_t s);
hipError_t radius_count_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, double radius, uint32_t* d_counts,
                               unsigned long long* d_offsets, hipStream_t s);
hipError_t radius_fill_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, double radius, const unsigned long long* d_offsets,
                              int64_t* d_idx, double* d_d2, hipStream_t s);
hipError_t radius_sort_launch(size_t n_q, const unsigned long long* d_offsets, const int64_t* d_in_idx, const double* d_in_d2, int64_t* d_out_idx,
                              double* d_out_d2, hipStream_t s);
// (the exclusive scan of the counts alone: d_offsets[i] = d_counts[0] + ... + d_counts[i - 1], i = 0 .. n_q)
hipError_t radius_scan_launch(const uint32_t* d_counts, size_t n_q, unsigned long long* d_offsets, hipStream_t s);

// ---------------------------------------------------------------------------
// Sparse target index (sparse_index.hip; the walk: sparse_walk.h): the same two queries on a target whose box no dense table can hold
// ---------------------------------------------------------------------------
static constexpr double kSparseCell = 1.0;      // cell edge of the sparse index (a power of two: x / cell is exact)
// what the build's last launch reports into page-locked memory: the points stored (the finite rows), the key layout and its verdict
struct SiResult { uint32_t kept; int32_t pad_; sw::Layout lay; };
struct SiBuffers {           // the build's scratch, all of it sized by n and freed after the build
    void* hdr;               // 256 bytes
    unsigned long long* key[2]; uint32_t* row[2];
    uint32_t* hist;          // key_sort_hist_bytes(n)
};
// d_keys (n x 8 bytes) / d_pts (n x 16 bytes): the index, in key order, entries [0, kept)
hipError_t sparse_index_build_launch(const SiBuffers& b, const float* d_src, size_t stride_floats, size_t n, unsigned long long* d_keys, sw::Point* d_pts,
                                     SiResult* result_mapped, hipStream_t s);
hipError_t knn_sparse_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, int k, int64_t* d_idx, double* d_d2, hipStream_t s);
hipError_t radius_sparse_count_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, double radius, uint32_t* d_counts,
                                      unsigned long long* d_offsets, hipStream_t s);
hipError_t radius_sparse_fill_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, double radius, const unsigned long long* d_offsets,
                                     int64_t* d_idx, double* d_d2, hipStream_t s);

// pcl::VoxelGrid on the device (voxel_filter.hip); grid must have been built with pcl_mode = 1
// (two launches queued behind the build; they read the header themselves and do nothing when it says overflow, stale or empty.  d_inten: n floats,
//  d_sums: n / 2048 + 2 words, d_wave: voxel_filter_wave_bytes(n); result_mapped: page-locked host memory the last block writes -- valid once the stream has been synchronised)
struct VfResult { uint32_t count; int32_t overflow, too_fine, stale, empty; uint32_t pad_; unsigned long long n_cells; };
size_t voxel_filter_wave_bytes(size_t n);
hipError_t voxel_filter_launch(const GridIndex& grid, const float* d_orig, size_t stride_floats, size_t n, uint32_t* d_inten, uint32_t* d_sums,
                               void* d_wave, float* d_out, size_t out_capacity, void* result_mapped, hipStream_t s);

// A scan's motion distortion undone (deskew.hip; the arithmetic and the table's layout: deskew_math.h).  One launch, one point per lane.  pts, times
// (or nullptr: the field at time_off of every record) and out are device memory, out == pts or disjoint from both; tab: K records of 8 doubles;
// counts: three words (before, after, nonfinite) the launch ADDS to; Rr / pr: the trajectory at the reference time.
struct DeskewArgs {
    const char* pts; const char* times; char* out; const double* tab; unsigned long long* counts;
    unsigned long long n;
    uint32_t stride, time_off;
    int32_t kind, K;
    double t0, Rr[9], pr[3];
};
constexpr unsigned long long kDeskewMaxPoints = 0x7fffffffull * 256;      // (the grid's x extent times the block)
hipError_t deskew_launch(const DeskewArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// Sparse voxel filters (voxel_sparse.hip): pcp::VoxelDownSampleV3 / V2 by a stable radix sort of packed voxel keys
// ---------------------------------------------------------------------------
static constexpr int kVsV3 = 3, kVsV2 = 2;                       // PCR_VOXEL_SPARSE_V3 / _V2
static constexpr int kVsRefusedRange = 1, kVsRefusedBits = 2;    // VsResult::refused
// what the filter's last launch reports into page-locked memory: the voxels emitted, the rows kept (finite), the digit passes the sort took
// (the sorted pairs lie in pair buffer `passes & 1`), the verdict and the three extents the key was laid out for
struct VsResult { uint32_t count, kept; int32_t passes, refused, bits; int32_t pad_; unsigned long long ext[3]; };
struct VsBuffers {           // device memory of one call, all of it sized by n (voxel_sparse_bytes)
    void* hdr;               // the call's header: box, key layout, counts
    unsigned long long* key[2]; uint32_t* row[2];      // the (key, row) pairs, sorted from one into the other digit by digit
    uint32_t* hist;          // per digit pass: [bin][tile] counts, scanned in place
    uint32_t* cnt;           // per sorted row: the rows of the voxel it starts if that voxel is emitted, else 0
    uint32_t* first;         // per wave of 64 sorted rows: its first voxel start (64: none)
    void* lead;              // per wave: the double sums in front of that start (V3)
    uint32_t* tile;          // per block of 256 sorted rows: voxels emitted, scanned in place
};
struct VsSizes { size_t hdr, key, row, hist, cnt, first, lead, tile; };
// ... and its stable radix sort of (64-bit key, row) pairs on its own (voxel_sparse.hip: key_sort_launch says what goes in and comes out): device
// memory by the number of pairs alone.  The control block lives in device memory: the launch in front of the sort sets `passes` there.
static constexpr uint32_t kVsDropped = 0xffffffffu;      // row number of a pair that leaves in the first pass (a non-finite row; rows end at 0xfffffff0)
struct KeySortCtl { uint32_t kept; int32_t passes; };
size_t key_sort_hist_bytes(size_t n);
void key_sort_launch(KeySortCtl* d_ctl, size_t n, unsigned long long* const key[2], uint32_t* const row[2], uint32_t* hist, hipStream_t s);
VsSizes voxel_sparse_bytes(size_t n);
hipError_t voxel_sparse_launch(const VsBuffers& b, const float* d_pts, size_t stride_floats, size_t n, float leaf, int kind, int max_voxel_pts,
                               int min_voxel_pts, float* d_out, size_t out_capacity, VsResult* result_mapped, hipStream_t s);

// ---------------------------------------------------------------------------
// NDT (ndt.hip)
// ---------------------------------------------------------------------------
struct NdtVoxel {            // VoxelGridCovariance::Leaf (pclomp/voxel_grid_covariance_omp.h:98-193): mean_, icov_
    double mean[3];
    double icov[9];          // row-major
    int32_t n, pad;
};
struct NdtPose { float R[9]; float t[3]; };              // final_transformation_ (Matrix4f), row-major R
struct NdtAngles {           // computeAngleDerivatives (ndt_omp_impl.hpp:289-395)
    float j[8][3], h[15][3];         // float tables j_ang / h_ang
    double jd[8][3], hd[15][3];      // double vectors j_ang_a_.. / h_ang_a2_..
};
struct NdtArgs {
    const float* src; uint32_t n_src, src_stride;
    const GridHeader* hdr;
    const uint32_t* vox_slot;
    const NdtVoxel* vox;
    double d1, d2;           // gauss_d1_, gauss_d2_ (ndt_omp_impl.hpp:86-93)
    double* partials;        // [blocks][48]
    int32_t use_tile;        // sharded target: only source points whose transformed position lies in [tile_lo, tile_hi)
    int32_t search;          // pcr_params.ndt_search (PCR_NDT_DIRECT*): read by the HOST launchers only, which pick the kernel instantiation by it
    double tile_lo[3], tile_hi[3];
    uint32_t* roi_escapes;   // target prepared for one scan (RoiView): count of lookups that hit a voxel it was not prepared for; else NULL
    uint32_t* pair_count;    // profiling passes only (pcr_set_profile >= 2), else NULL: [32] += (point, voxel) pairs of gradient-only passes, [48] += of passes with a Hessian
};
hipError_t ndt_launch_voxels(const GridIndex& grid, uint32_t* d_slot, NdtVoxel* d_vox, uint32_t* d_count, uint32_t* d_count_next, uint32_t* d_list, size_t list_capacity,
                             int min_points, double eig_mult, hipStream_t s, const RoiView* roi = nullptr, bool listed_by_tile_pass = false);
hipError_t ndt_launch_derivatives(const NdtArgs& a, const NdtPose& T, const NdtAngles& ang, int compute_hessian, double* d_out48, hipStream_t s, double seq = 0.0);
hipError_t ndt_launch_hessian(const NdtArgs& a, const NdtPose& T, const NdtAngles& ang, double* d_out48, hipStream_t s, double seq = 0.0);
// device-resident optimiser (ndt_opt.h): controller state in HBM, result in host-mapped memory
struct NdtCtl;
struct NdtOut;
hipError_t ndt_launch_ctl_init(NdtCtl* d_ctl, const NdtPose& T0, const double p[6], double step_size, double trans_eps, int max_iters, hipStream_t s, int no_replay = 0,
                               uint32_t* d_roi_escapes = nullptr);
hipError_t ndt_launch_ctl_state(NdtCtl* d_ctl, const NdtCtl& c, hipStream_t s, uint32_t* d_roi_escapes = nullptr);
void ndt_ctl_init_blob(BlobStore* b, NdtCtl* d_ctl, const NdtPose& T0, const double p[6], double step_size, double trans_eps, int max_iters, int no_replay_arg);
hipError_t ndt_launch_pass_pro(const NdtArgs& a, NdtCtl* d_ctl2, double* d_rows2, NdtOut* d_out, hipStream_t s, double seq, int index,
                               hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t ndt_launch_pass_fold(const NdtArgs& a, NdtCtl* d_ctl, double* d_sums48, hipStream_t s);
hipError_t ndt_launch_ctl(const NdtArgs& a, NdtCtl* d_ctl, const double* d_sums48, NdtOut* d_out, hipStream_t s, double seq, int batch_mark);
struct PeerComm;
hipError_t ndt_launch_pass_peer(const NdtArgs& a, NdtCtl* d_ctl, const PeerComm& pc, double xseq, NdtOut* d_out, hipStream_t s, double seq);
uint32_t ndt_blocks(uint32_t n_src);

// peer exchange (loam.hip): receive buffers of all ranks as THIS process maps them
static constexpr int kMaxPeers = 8;
static constexpr int kPeerSlot = 72;                       // doubles per (parity, writer) slot: 64 values + the sequence word + padding
static constexpr int kPeerFlag = 64;
static constexpr unsigned long long kPeerTimeoutTicks = 200000000ull;      // 2 s of the 100 MHz clock
struct PeerComm { double* buf[kMaxPeers]; int32_t rank, nranks; int32_t* status; };      // status: host-mapped word, set to 1 by an exchange that timed out (out of band: the sums may hold any value, NaN included)
hipError_t loam_launch_peer_exchange(const LoamArgs& a, int k, const PeerComm& pc, double seq, double* d_out, hipStream_t s);
hipError_t peer_launch_allreduce(double* d_inout, int n, int op, const PeerComm& pc, double seq, hipStream_t s);
hipError_t loam_launch_iteration(const LoamArgs& a, int k, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t loam_launch_finalize(const LoamArgs& a, int k, hipStream_t s);
hipError_t loam_launch_reduce(const LoamArgs& a, int k, double* d_out, hipStream_t s);
uint32_t loam_grid_blocks(uint32_t n_src);

}  // namespace pcr

// (library-internal, not part of the C ABI) the stream a handle queues its work on: the sub-map assembly queues its transform pass in front of the
// voxel filter it runs through a handle, on that handle's stream, so that one synchronisation serves both
struct pcr_handle;
hipStream_t pcr_internal_stream(const pcr_handle* h);
// ... and the voxel filter in two halves, device memory into device memory (out_capacity >= n): queue it; synchronise and collect it (redone there if the index's hints did not hold)
int pcr_internal_vf_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity);
int pcr_internal_vf_end(pcr_handle* h, size_t* n_out);
// ... and a hint: clouds of up to `points` points will come (the filter's and its index's buffers are sized for that at the next call)
void pcr_internal_vf_reserve(pcr_handle* h, size_t points);
