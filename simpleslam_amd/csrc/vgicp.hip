// vgicp.hip -- voxelised GICP scan-to-map on gfx950 (hand-written HIP).
//
// Kernels for the reference's PCR::VgicpRegister::scan2Map (PCR/src/VgicpRegister.cpp:30-45),
// i.e. fast_gicp::FastVGICP under PCL's align():
//   V2 per-point covariances      fast_gicp_impl.hpp:241-297  (serial there: 20-NN over a FLANN
//      kd-tree, 4x20 f64 neighbours, cov/20, JacobiSVD, the regularisation: PLANE U diag(1,1,1e-3) V^T by default,
//      pcr_params.vgicp_regularization for the other four of fast_gicp_impl.hpp:263-293)
//      -> vgicp_cov_kernel: exact ring search on the uniform grid, float distances like FLANN
//   V3 Gaussian voxel map         pclomp/fast_vgicp_voxel.hpp:79-174 (serial unordered_map; ADDITIVE by default, MULTIPLICATIVE by
//      pcr_params.vgicp_voxel_mode)
//      -> vgicp_voxel_kernel: one thread per voxel, fixed-point sums (order independent)
//   V4/V5 correspondences, Mahalanobis, linearize, compute_error   fast_vgicp_impl.hpp:73-204
//      -> vgicp_linearize_kernel<false, kSearch> (linearize) and <true, kSearch> (compute_error of an LM trial pose + the linearisation at
//         that pose in the same pass), fixed-order reductions; kSearch = pcr_params.vgicp_search: DIRECT1 one voxel per point, DIRECT7 /
//         DIRECT27 every occupied voxel of the 7 / 27 cells around it (fast_vgicp_voxel.hpp:10-44)
//   V6 LM driver                  lsq_registration_impl.hpp:53-171 -> lsq_pass.h (the pass and the device loop's prologue), lsq_host.h: run_lsq
// Also the PCL fitness score (pcl::Registration::getFitnessScore, VgicpRegister.cpp:42-45).
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "peer_exchange.h"
#include "small_math.h"
#include "vgicp_opt.h"
#include "lsq_pass.h"
#include "cov_math.h"
#include "ring_search.h"

namespace pcr {

// kBatch: ring 1 of every level with its nine row ranges requested at once (ring_level).  For a SCAN-sized cloud, whose search is a chain
// of dependent round trips at one wave per SIMD: A/B on one box, the scan's 65 k covariances no longer hold the optimiser up (align 0.19 ->
// 0.11 ms).  A map-sized cloud runs the same kernel at four waves per SIMD and is bound by instruction issue: there the batched form
// costs 0.83 -> 1.28 ms per million points, so it keeps the row-by-row walk.
// A map-sized target prepared for one scan: the sorted positions of the points whose voxel the scan can reach, compacted (in blocks of 1 024
// positions, each block's share in order; one atomic per block).  The covariance kernel below then runs FULL waves over the region's ~100 k points
// instead of 16 000 thin ones over the million, most of whose lanes left at the region test while the others searched.
__global__ __launch_bounds__(256) void vgicp_region_list_kernel(GridView g, uint32_t n_sorted_max, const RoiView roi, uint32_t* __restrict__ list,
                                                                uint32_t* __restrict__ count, uint32_t* __restrict__ count_next) {
    __shared__ uint32_t sh_cnt[16], sh_base;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_next = 0u;      // (the other of two counters, for the next call: before anything can return)
    const GridHeader h = *g.hdr;
    if (h.empty || h.overflow || h.stale) return;
    const GridHeader lat = *roi.lat;
    if (lat.stale || lat.overflow) return;
    const uint32_t n = min(g.cell_start[h.n_cells], n_sorted_max);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c0 = blockIdx.x * 1024u; c0 < n; c0 += gridDim.x * 1024u) {
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t j = c0 + (uint32_t)u * 256u + threadIdx.x;
            bool in = false;
            if (j < n) { const float4 q = g.pts[j]; in = roi_holds_point(roi, lat, (double)q.x, (double)q.y, (double)q.z); }
            m[u] = __ballot(in);
            if (lane == 0) sh_cnt[u * 4 + wave] = (uint32_t)__popcll(m[u]);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int k = 0; k < 16; ++k) tot += sh_cnt[k];
            sh_base = tot ? atomicAdd(count, tot) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint32_t off = sh_base;
            for (int k = 0; k < u * 4 + wave; ++k) off += sh_cnt[k];
            if ((m[u] >> lane) & 1ull) list[off + (uint32_t)__popcll(m[u] & ((1ull << lane) - 1ull))] = c0 + (uint32_t)u * 256u + threadIdx.x;
        }
        __syncthreads();      // sh_cnt is rewritten by the next chunk
    }
}

// list / list_count (optional): the sorted positions to process (vgicp_region_list_kernel) instead of every position with the region test
// kReg: the regularisation (PCR_REG_*), a template parameter of the arithmetic (cov_math.h), chosen on the host
template <bool kBatch, int kReg>
__global__ __launch_bounds__(256, kBatch ? 1 : 4) void vgicp_cov_kernel(GridView g, GridView g1, GridView g2, int n_levels, const float* __restrict__ orig,
                                                        uint32_t stride, uint32_t n_sorted_max, double* __restrict__ cov6, const int use_check,
                                                        const CovCheck chk, const RoiView roi, const uint32_t* __restrict__ list,
                                                        const uint32_t* __restrict__ list_count) {
    __shared__ uint2 sh_rows[kBatch ? 9 * 256 : 1];      // row ranges of ring 1 (ring_level)
    const GridHeader h = *g.hdr;
    if (h.empty || h.overflow || h.stale) return;      // (stale: queued ahead of the host's look at the header, capi.hip: settle_cov_levels; the caller builds afresh)
    GridHeader lat;
    if (roi.mask) lat = *roi.lat;
    if (roi.mask && (lat.stale || lat.overflow)) return;
    GridLevels lv;
    lv.hdr[0] = g.hdr; lv.pts[0] = g.pts; lv.cell_start[0] = g.cell_start;
    lv.hdr[1] = g1.hdr; lv.pts[1] = g1.pts; lv.cell_start[1] = g1.cell_start;
    lv.hdr[2] = g2.hdr; lv.pts[2] = g2.pts; lv.cell_start[2] = g2.cell_start;
    lv.n = n_levels;
    if (n_levels > 1 && (g1.hdr->overflow || g1.hdr->empty)) lv.n = 1;
    if (n_levels > 2 && (g2.hdr->overflow || g2.hdr->empty)) lv.n = min(lv.n, 2);
    const uint32_t n = list ? *list_count : min(g.cell_start[h.n_cells], n_sorted_max);   // points actually indexed (finite ones), or the listed ones
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t j = list ? list[i] : i;
        const float4 q = g.pts[j];
        // a target prepared for one scan: only the points whose voxel the scan can reach (the search itself always sees the whole cloud)
        if (!list && roi.mask && !roi_holds_point(roi, lat, (double)q.x, (double)q.y, (double)q.z)) continue;
        if (roi.count) atomicAdd(roi.count, 1u);      // (profiling passes only)
        KeyList<kCovK> L;
        ring_knn<kCovK>(lv, q.x, q.y, q.z, 3.0e38f, L, kBatch ? sh_rows : nullptr);
        uint32_t nb_idx[kCovK];
#pragma unroll
        for (int i = 0; i < kCovK; ++i) nb_idx[i] = L.k[i] != ~0ull ? (uint32_t)L.k[i] : 0xffffffffu;
        const int found = cov_from_neighbours<kReg>(nb_idx, orig, stride, cov6 + (size_t)__float_as_uint(q.w) * 6);
        if (use_check) {
            // sharded target: this rank holds every map point inside [ext_lo, ext_hi) only.  The neighbourhood of a point that
            // can enter a voxel of the tile is the map's own iff its 20th neighbour is nearer than every face of that region.
            const double qd[3] = {(double)q.x, (double)q.y, (double)q.z};
            bool in = true;
            double margin = 1e300;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                in = in && qd[d] >= chk.chk_lo[d] && qd[d] < chk.chk_hi[d];
                margin = fmin(margin, fmin(qd[d] - chk.ext_lo[d], chk.ext_hi[d] - qd[d]));
            }
            if (in && margin < 1e29) {
                const double r20 = found == kCovK ? sqrt((double)__uint_as_float((uint32_t)(L.k[kCovK - 1] >> 32))) * (1.0 + 1e-6) : 1e300;
                if (!(r20 < margin)) atomicAdd(chk.violations, 1u);
            }
        }
    }
}

// ------------------------------------------------------------------------------
// V3: Gaussian voxel map.  Reference voxel coordinate c = floor(x/res - 0.5)
// (fast_vgicp_voxel.hpp:158-160): the target index is built on exactly that lattice
// (GridHeader.shift = 0.5), so a voxel IS a cell and its points are one contiguous run.
// One thread per sorted point; the thread of a cell's first point folds the run and stores the
// voxel at that position (no slot table, no counter).
// Sums are fixed point (2^44 per unit, or a scale chosen per voxel: fold_scaled), hence independent of the order of the points.
// ------------------------------------------------------------------------------
static constexpr double kFix = 17592186044416.0;   // 2^44

__device__ __forceinline__ bool lattice_key(const GridHeader& h, double x, double y, double z, uint32_t* key, double c[3]) {
    c[0] = floor(x / h.cell - h.shift); c[1] = floor(y / h.cell - h.shift); c[2] = floor(z / h.cell - h.shift);
    const double vx = c[0] - h.org[0], vy = c[1] - h.org[1], vz = c[2] - h.org[2];
    if (!(vx >= 0.0 && vx < (double)h.dims[0] && vy >= 0.0 && vy < (double)h.dims[1] && vz >= 0.0 && vz < (double)h.dims[2])) return false;
    *key = ((uint32_t)vz * (uint32_t)h.dims[1] + (uint32_t)vy) * (uint32_t)h.dims[0] + (uint32_t)vx;
    return true;
}

// ---- the fold beyond unit covariances ----
// The fixed scale 2^44 is exact only while the terms stay below 1: PLANE and NORMALIZED_MIN_EIG under ADDITIVE.  Every other setting has terms
// without a bound (the scatter itself; FROBENIUS up to (w_max + 1e-3) / 1e-3; an inverse covariance up to 1e3 and beyond), so the scale is
// chosen per voxel: a first pass over the run takes the largest magnitude m of the terms (a maximum does not depend on the order); with e the
// smallest exponent with m <= 2^e and c = ceil(log2 cnt), every term is rounded to a multiple of 2^-s, s = 62 - e - c, and added as a long long:
// a term is at most 2^(62 - c), a sum at most 2^62.  The integer sums are exact, hence independent of the order; a term loses at most
// 2^(c - 63) of the largest one, which for a thousand points is the rounding of a double.  A term that is not finite makes the voxel's
// covariance NaN: it never reaches the integer conversion.
enum { kFoldFixed = 0, kFoldScaled = 1, kFoldMult = 2 };

__device__ __forceinline__ int fold_scale(double m, uint32_t cnt) {
    int e = 0;
    if (m != 0.0 && frexp(m, &e) == 0.5) --e;      // m <= 2^e, the smallest such e
    const int c = cnt > 1u ? 32 - __clz((int)(cnt - 1u)) : 0;      // cnt <= 2^c
    return 62 - e - c;
}

// one point's terms: ADDITIVE the covariance's six entries and the offset from the voxel's corner; MULTIPLICATIVE A = C^-1 (the 3x3 block of the
// reference's 4x4 with (3,3) = 1, which is block diagonal: fast_vgicp_voxel.hpp:86-94) and B = A (p - corner)
template <bool kMult>
__device__ __forceinline__ void fold_terms(const float4& p, const double* __restrict__ cc, const double o[3], double A[6], double B[3]) {
    const double d[3] = {(double)p.x - o[0], (double)p.y - o[1], (double)p.z - o[2]};
    if constexpr (kMult) {
        const double C[6] = {cc[0], cc[1], cc[2], cc[3], cc[4], cc[5]};
        inv3_sym(C, A);
        B[0] = A[0] * d[0] + A[1] * d[1] + A[2] * d[2]; B[1] = A[1] * d[0] + A[3] * d[1] + A[4] * d[2]; B[2] = A[2] * d[0] + A[4] * d[1] + A[5] * d[2];
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = cc[k];
        B[0] = d[0]; B[1] = d[1]; B[2] = d[2];
    }
}

template <bool kMult>
__device__ __forceinline__ void fold_scaled(const GridView& g, const double* __restrict__ cov6, uint32_t j, uint32_t e, const double o[3], VgicpVoxel& v) {
    const uint32_t cnt = e - j;
    double mA = 0.0, mB = 0.0;
    bool badA = false, badB = false;
    for (uint32_t i = j; i < e; ++i) {
        const float4 p = g.pts[i];
        double A[6], B[3];
        fold_terms<kMult>(p, cov6 + (size_t)__float_as_uint(p.w) * 6, o, A, B);
#pragma unroll
        for (int k = 0; k < 6; ++k) { const double t = fabs(A[k]); badA = badA || !(t <= DBL_MAX); mA = fmax(mA, t); }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double t = fabs(B[k]); badB = badB || !(t <= DBL_MAX); mB = fmax(mB, t); }
    }
    const double qnan = __builtin_nan("");
    const int sA = badA ? 0 : fold_scale(mA, cnt), sB = badB ? 0 : fold_scale(mB, cnt);
    long long a[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (uint32_t i = j; i < e; ++i) {
        const float4 p = g.pts[i];
        double A[6], B[3];
        fold_terms<kMult>(p, cov6 + (size_t)__float_as_uint(p.w) * 6, o, A, B);
        if (!badA) {
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] += llrint(ldexp(A[k], sA));
        }
        if (!badB) {
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] += llrint(ldexp(B[k], sB));
        }
    }
    double SA[6], SB[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) SA[k] = badA ? qnan : ldexp((double)a[k], -sA);
#pragma unroll
    for (int k = 0; k < 3; ++k) SB[k] = badB ? qnan : ldexp((double)b[k], -sB);
    if constexpr (kMult) {
        // finalize (fast_vgicp_voxel.hpp:96-102): cov = (sum A)^-1, mean = cov * sum A p = corner + cov * sum A (p - corner)
        inv3_sym(SA, v.cov);
        v.mean[0] = o[0] + (v.cov[0] * SB[0] + v.cov[1] * SB[1] + v.cov[2] * SB[2]);
        v.mean[1] = o[1] + (v.cov[1] * SB[0] + v.cov[3] * SB[1] + v.cov[4] * SB[2]);
        v.mean[2] = o[2] + (v.cov[2] * SB[0] + v.cov[4] * SB[1] + v.cov[5] * SB[2]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) v.mean[k] = o[k] + SB[k] / (double)cnt;
#pragma unroll
        for (int k = 0; k < 6; ++k) v.cov[k] = SA[k] / (double)cnt;
    }
}

// kFold: kFoldFixed = ADDITIVE over covariances with entries <= 1 (PLANE, NORMALIZED_MIN_EIG): the fixed scale below; kFoldScaled = ADDITIVE over
// any covariances, kFoldMult = MULTIPLICATIVE: a scale per voxel (fold_scaled)
template <int kFold>
__global__ __launch_bounds__(256) void vgicp_voxel_kernel(GridView g, const double* __restrict__ cov6, VgicpVoxel* __restrict__ vox, const RoiView roi) {
    const GridHeader h = *g.hdr;
    if (h.overflow || h.empty || h.stale) return;
    const uint32_t n = g.cell_start[h.n_cells];
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const float4 q = g.pts[j];
        uint32_t key;
        double c[3];
        if (!lattice_key(h, (double)q.x, (double)q.y, (double)q.z, &key, c)) continue;
        if (g.cell_start[key] != j) continue;                 // not the first point of its voxel
        if (roi.mask && roi.mask[roi_macro(h, roi.mshift, (int)(c[0] - h.org[0]), (int)(c[1] - h.org[1]), (int)(c[2] - h.org[2]))] == 0) continue;      // out of the scan's reach
        if (roi.count) atomicAdd(roi.count + 16, 1u);      // (profiling passes only)
        const uint32_t e = g.cell_start[key + 1];
        const double ox = (c[0] + h.shift) * h.cell, oy = (c[1] + h.shift) * h.cell, oz = (c[2] + h.shift) * h.cell;   // lower corner
        const uint32_t cnt = e - j;
        VgicpVoxel v;
        if constexpr (kFold != kFoldFixed) {
            const double o[3] = {ox, oy, oz};
            fold_scaled<kFold == kFoldMult>(g, cov6, j, e, o, v);
        } else {
            const double inv = 1.0 / (double)cnt;
            // Every term is rounded to a multiple of 2^-44 first, so the sums are exact and independent of the order.  While they provably
            // stay below 2^53 (offsets < cell, covariance entries <= 1 in magnitude after the regularisation) the integers are added
            // up as doubles -- one v_rndne_f64 and one v_add_f64 per term, where the f64 -> i64 conversion alone costs a dozen instructions.
            if ((double)cnt * (h.cell > 1.0 ? h.cell : 1.0) <= 256.0) {
                double dm[3] = {0, 0, 0}, dc[6] = {0, 0, 0, 0, 0, 0};
                for (uint32_t i = j; i < e; ++i) {
                    const float4 p = g.pts[i];
                    dm[0] += rint(((double)p.x - ox) * kFix); dm[1] += rint(((double)p.y - oy) * kFix); dm[2] += rint(((double)p.z - oz) * kFix);
                    const double* cc = cov6 + (size_t)__float_as_uint(p.w) * 6;
#pragma unroll
                    for (int k = 0; k < 6; ++k) dc[k] += rint(cc[k] * kFix);
                }
                v.mean[0] = ox + dm[0] / kFix * inv; v.mean[1] = oy + dm[1] / kFix * inv; v.mean[2] = oz + dm[2] / kFix * inv;
#pragma unroll
                for (int k = 0; k < 6; ++k) v.cov[k] = dc[k] / kFix * inv;
            } else {
                long long sm[3] = {0, 0, 0}, sc[6] = {0, 0, 0, 0, 0, 0};
                for (uint32_t i = j; i < e; ++i) {
                    const float4 p = g.pts[i];
                    sm[0] += llrint(((double)p.x - ox) * kFix); sm[1] += llrint(((double)p.y - oy) * kFix); sm[2] += llrint(((double)p.z - oz) * kFix);
                    const double* cc = cov6 + (size_t)__float_as_uint(p.w) * 6;
#pragma unroll
                    for (int k = 0; k < 6; ++k) sc[k] += llrint(cc[k] * kFix);
                }
                v.mean[0] = ox + (double)sm[0] / kFix * inv; v.mean[1] = oy + (double)sm[1] / kFix * inv; v.mean[2] = oz + (double)sm[2] / kFix * inv;
#pragma unroll
                for (int k = 0; k < 6; ++k) v.cov[k] = (double)sc[k] / kFix * inv;
            }
        }
        v.w = sqrt((double)cnt);   // fast_vgicp_impl.hpp:149
        v.n = cnt; v.pad = 0;
        vox[j] = v;
    }
}

// ------------------------------------------------------------------------------
// V4/V5: one linearisation (update_correspondences + linearize)
// ------------------------------------------------------------------------------
// roi: a voxel that exists but lies outside the prepared region is an ESCAPE (counted; the host prepares the whole target and repeats)
__device__ __forceinline__ uint32_t vgicp_lookup(const GridHeader& h, const uint32_t* __restrict__ cell_start, const double tp[3], const RoiView& roi) {
    if (h.overflow || h.empty) return 0;
    uint32_t key;
    double c[3];
    if (!lattice_key(h, tp[0], tp[1], tp[2], &key, c)) return 0;
    // (an index of the region's points only -- roi.filtered -- holds nothing outside the mask, not even the cell table's entries: the mask is tested
    //  FIRST, and a lookup outside it is an escape whether or not a voxel is there -- as NDT treats its region-only index)
    const bool outside = roi.mask && roi.mask[roi_macro(h, roi.mshift, (int)(c[0] - h.org[0]), (int)(c[1] - h.org[1]), (int)(c[2] - h.org[2]))] == 0;
    if (outside && roi.filtered) { atomicAdd(roi.escapes, 1u); return 0; }
    const uint32_t s = cell_start[key], e = cell_start[key + 1];
    if (e > s && outside) {
        atomicAdd(roi.escapes, 1u);
        return 0;
    }
    return e > s ? s + 1 : 0;
}

// ------------------------------------------------------------------------------
// neighbourhood (pcr_params.vgicp_search; fast_vgicp_voxel.hpp:10-44, fast_vgicp_impl.hpp:73-116): kSearch is a template parameter of the
// per-point functions, of VgicpPass and of the kernels that hold them, chosen on the host (VGICP_SEARCH_DISPATCH).
//   DIRECT1   the point's own voxel: the code this unit had before the setting (vgicp_lookup, one slot and one M per point)
//   DIRECT7   table: centre, +x -x +y -y +z -z          DIRECT27   table: {-1, 0, 1}^3, x outermost, z fastest, the centre INCLUDED
// Under DIRECT7 / DIRECT27 a point has up to K = 7 / 27 pairs, one per table entry k whose voxel c + d_k exists; c + d_k is tested against
// the lattice box per axis, so a point whose own cell lies one layer outside the box still reaches the box's outer voxels.
// Two steps per point.  The LOOKUP walks the rows of the block -- the cell table is dense with x fastest, so the three cells of an x-row are four
// adjacent words -- and leaves slot + 1 (0: none) of entry k at corr_slot[k][i] and the presence bits at corr_slot[K][i]: [K + 1][n_src], every
// store and every later load coalesced over the wave.  The PAIR LOOP takes the set bits lowest first, which IS table order, and adds each
// pair's terms into the thread's 28 sums; it is not unrolled (27 copies of the body would not fit the instruction cache).
// Storage: M is NOT kept per pair.  DIRECT27 would write 27 x 48 B per point and pass (85 MB for a 65 536-point scan, twice that allocated for
// the two buffer pairs) and read it back in compute_error; M = (C_B + T0 C_A T0^T)^-1 costs ~60 flops from the voxel record compute_error reads
// anyway (its mean and weight share the record with C_B).  So the linearisation leaves its pose T0 beside its slots (corr_T) and
// compute_error derives M again: T0 C_A T0^T once per point, one 3 x 3 inverse per pair.
// ------------------------------------------------------------------------------
template <int kSearch> constexpr int kVgPairs = kSearch == PCR_VGICP_DIRECT27 ? 27 : kSearch == PCR_VGICP_DIRECT7 ? 7 : 1;

// the table entry of offset (dx, dy, dz), -1 when the table has none (constant after unrolling)
template <int kSearch>
__device__ __forceinline__ constexpr int vg_entry(int dx, int dy, int dz) {
    if (kSearch == PCR_VGICP_DIRECT27) return (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1);
    if (dx == 0 && dy == 0 && dz == 0) return 0;
    if (kSearch != PCR_VGICP_DIRECT7) return -1;
    if (dy == 0 && dz == 0) return dx > 0 ? 1 : 2;
    if (dx == 0 && dz == 0) return dy > 0 ? 3 : 4;
    if (dx == 0 && dy == 0) return dz > 0 ? 5 : 6;
    return -1;
}
// ... and the offset of entry k
template <int kSearch>
__device__ __forceinline__ void vg_offset(int k, int d[3]) {
    if constexpr (kSearch == PCR_VGICP_DIRECT27) {
        const int kx = k / 9, r = k - kx * 9, ky = r / 3;
        d[0] = kx - 1; d[1] = ky - 1; d[2] = r - ky * 3 - 1;
    } else {
        const int axis = (k - 1) >> 1, sgn = (k & 1) ? 1 : -1;      // 1 +x, 2 -x, 3 +y, 4 -y, 5 +z, 6 -z; 0: the centre (axis = -1)
        d[0] = axis == 0 ? sgn : 0; d[1] = axis == 1 ? sgn : 0; d[2] = axis == 2 ? sgn : 0;
    }
}

// the centre cell of a transformed point in the box's coordinates, or (-4, -4, -4) -- from where no table entry reaches the box -- when the index
// holds nothing or the point lies more than one layer outside
__device__ __forceinline__ void vg_centre(const GridHeader& h, const double tp[3], int c[3]) {
    const double fx = floor(tp[0] / h.cell - h.shift) - h.org[0], fy = floor(tp[1] / h.cell - h.shift) - h.org[1], fz = floor(tp[2] / h.cell - h.shift) - h.org[2];
    const bool ok = !(h.overflow || h.empty) && fx >= -1.0 && fx <= (double)h.dims[0] && fy >= -1.0 && fy <= (double)h.dims[1] && fz >= -1.0 && fz <= (double)h.dims[2];
    c[0] = ok ? (int)fx : -4; c[1] = ok ? (int)fy : -4; c[2] = ok ? (int)fz : -4;
}

// the lookup of one point: slot + 1 of every table entry to slot_out[k][i], the presence bits to slot_out[K][i] and back.  A neighbour outside a
// region-only mask is an escape exactly as a centre is (vgicp_lookup).
template <int kSearch>
__device__ __forceinline__ uint32_t vgicp_neighbours(const GridHeader& h, const uint32_t* __restrict__ cell_start, const int c[3], const RoiView& roi,
                                                     uint32_t i, uint32_t n_src, uint32_t* __restrict__ slot_out) {
    constexpr int K = kVgPairs<kSearch>;
    const int d0 = h.dims[0], d1 = h.dims[1], d2 = h.dims[2];
    uint32_t mask = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const bool side = vg_entry<kSearch>(-1, dy, dz) >= 0 || vg_entry<kSearch>(1, dy, dz) >= 0;
            if (!side && vg_entry<kSearch>(0, dy, dz) < 0) continue;      // (a row DIRECT7's table does not touch)
            const int y = c[1] + dy, z = c[2] + dz;
            const bool row_ok = y >= 0 && y < d1 && z >= 0 && z < d2;
            const uint32_t base = ((uint32_t)z * (uint32_t)d1 + (uint32_t)y) * (uint32_t)d0;
            // the row's words c[0] - 1 .. c[0] + 2 of the cell table (the table has one entry past the last cell): cell x is [w[x - c[0] + 1], w[x - c[0] + 2])
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = side ? 0 : 1; j < (side ? 4 : 3); ++j) {
                const int x = c[0] - 1 + j;
                if (row_ok && x >= 0 && x <= d0) w[j] = cell_start[base + (uint32_t)x];
            }
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int k = vg_entry<kSearch>(dx, dy, dz);
                if (k < 0) continue;
                const int x = c[0] + dx;
                uint32_t slot = 0u;
                if (row_ok && x >= 0 && x < d0) {
                    const uint32_t s = w[dx + 1], e = w[dx + 2];
                    const bool outside = roi.mask && roi.mask[roi_macro(h, roi.mshift, x, y, z)] == 0;
                    // (a region-only index holds nothing outside the mask: there the words are not the whole target's, and the lookup is an escape
                    //  whether or not a voxel is there)
                    if (outside && (roi.filtered || e > s)) atomicAdd(roi.escapes, 1u);
                    else if (e > s) slot = s + 1u;
                }
                slot_out[(size_t)k * n_src + i] = slot;
                mask |= slot ? 1u << k : 0u;
            }
        }
    }
    slot_out[(size_t)K * n_src + i] = mask;
    return mask;
}

// T C_A T^T of a source point (upper triangle), the part of a pair's combined covariance that does not depend on the voxel
__device__ __forceinline__ void vg_rcr(const Pose16& T, const double* __restrict__ ca, double R6[6]) {
    const double CA[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
    double RC[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) RC[r][c] = T.m[r] * CA[0][c] + T.m[4 + r] * CA[1][c] + T.m[8 + r] * CA[2][c];
    int o = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) { R6[o] = RC[r][0] * T.m[c] + RC[r][1] * T.m[4 + c] + RC[r][2] * T.m[8 + c]; ++o; }
}

// update_correspondences + linearize of one source point over its pairs (DIRECT7, DIRECT27): every pair's terms added to v in table order
template <int kSearch>
__device__ __forceinline__ void vgicp_lin_pairs(const VgicpArgs& a, const GridHeader& h, const Pose16& T, uint32_t i, double v[28],
                                                uint32_t* __restrict__ slot_out, double* __restrict__ T_out) {
    if (i == 0) {      // the pose these pairs belong to, for compute_error (one thread of the launch)
#pragma unroll
        for (int k = 0; k < 16; ++k) T_out[k] = T.m[k];
    }
    const float* sp = a.src + (size_t)i * a.src_stride;
    const double p[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
    double tp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) tp[r] = T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0;
    int c[3];
    vg_centre(h, tp, c);
    if (a.use_tile && !(tp[0] >= a.tile_lo[0] && tp[0] < a.tile_hi[0] && tp[1] >= a.tile_lo[1] && tp[1] < a.tile_hi[1] &&
                        tp[2] >= a.tile_lo[2] && tp[2] < a.tile_hi[2])) c[0] = c[1] = c[2] = -4;      // (a query tile: the host refuses these settings on a sharded handle)
    uint32_t mask = vgicp_neighbours<kSearch>(h, a.cell_start, c, a.roi, i, a.n_src, slot_out);
    if (a.escapes && h.clamped) {
        // a cut index (vgicp_lin_point): guard_cells already holds the voxel these settings reach beyond the point's own
        const double cc[3] = {floor(tp[0] / h.cell - h.shift) - h.org[0], floor(tp[1] / h.cell - h.shift) - h.org[1], floor(tp[2] / h.cell - h.shift) - h.org[2]};
        const double g = (double)(kPad + a.guard_cells);
        bool esc = false;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            esc = esc || ((h.cut_mask & (1 << d)) && cc[d] < g) || ((h.cut_mask & (8 << d)) && cc[d] >= (double)h.dims[d] - g);
        if (esc) atomicAdd(a.escapes, 1u);
    }
    if (!mask) return;
    double R6[6];
    vg_rcr(T, a.src_cov6 + (size_t)i * 6, R6);
    // J = [skew(Tp) | -I]   fast_vgicp_impl.hpp:156-158, so3.hpp:21-31
    const double J[3][6] = {{0, -tp[2], tp[1], -1, 0, 0}, {tp[2], 0, -tp[0], 0, -1, 0}, {-tp[1], tp[0], 0, 0, 0, -1}};
#pragma unroll 1
    while (mask) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1u;
        int d[3];
        vg_offset<kSearch>(k, d);
        // (inside the box and occupied: the bit was set from this cell's words; read again from the cache)
        const uint32_t key = ((uint32_t)(c[2] + d[2]) * (uint32_t)h.dims[1] + (uint32_t)(c[1] + d[1])) * (uint32_t)h.dims[0] + (uint32_t)(c[0] + d[0]);
        const VgicpVoxel vx = a.vox[a.cell_start[key]];
        double S[6], M6[6];
#pragma unroll
        for (int o = 0; o < 6; ++o) S[o] = vx.cov[o] + R6[o];
        inv3_sym(S, M6);   // (C_B + T C_A T^T)^-1, fast_vgicp_impl.hpp:104-115
        const double M[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
        const double er[3] = {vx.mean[0] - tp[0], vx.mean[1] - tp[1], vx.mean[2] - tp[2]};
        double Me[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) Me[r] = M[r][0] * er[0] + M[r][1] * er[1] + M[r][2] * er[2];
        const double w = vx.w;
        double MJ[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) MJ[r][cc] = M[r][0] * J[0][cc] + M[r][1] * J[1][cc] + M[r][2] * J[2][cc];
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = r; cc < 6; ++cc) v[q++] += w * (J[0][r] * MJ[0][cc] + J[1][r] * MJ[1][cc] + J[2][r] * MJ[2][cc]);
#pragma unroll
        for (int r = 0; r < 6; ++r) v[21 + r] += w * (J[0][r] * Me[0] + J[1][r] * Me[1] + J[2][r] * Me[2]);
        v[27] += w * (er[0] * Me[0] + er[1] * Me[1] + er[2] * Me[2]);
    }
}

// compute_error of one point over the pairs of the LAST linearisation (DIRECT7, DIRECT27): its slots, and every M derived again from its pose
template <int kSearch>
__device__ __forceinline__ double vgicp_err_pairs(const VgicpArgs& a, const Pose16& T, uint32_t i) {
    constexpr int K = kVgPairs<kSearch>;
    uint32_t mask = a.corr_slot[(size_t)K * a.n_src + i];
    if (!mask) return 0.0;
    Pose16 T0;
#pragma unroll
    for (int k = 0; k < 16; ++k) T0.m[k] = a.corr_T[k];
    double R6[6];
    vg_rcr(T0, a.src_cov6 + (size_t)i * 6, R6);
    const float* sp = a.src + (size_t)i * a.src_stride;
    const double p[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
    double tp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) tp[r] = T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0;
    double sum = 0.0;
#pragma unroll 1
    while (mask) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1u;
        const VgicpVoxel vx = a.vox[a.corr_slot[(size_t)k * a.n_src + i] - 1u];
        double S[6], M6[6];
#pragma unroll
        for (int o = 0; o < 6; ++o) S[o] = vx.cov[o] + R6[o];
        inv3_sym(S, M6);
        const double er[3] = {vx.mean[0] - tp[0], vx.mean[1] - tp[1], vx.mean[2] - tp[2]};
        const double Me0 = M6[0] * er[0] + M6[1] * er[1] + M6[2] * er[2], Me1 = M6[1] * er[0] + M6[3] * er[1] + M6[4] * er[2],
                     Me2 = M6[2] * er[0] + M6[4] * er[1] + M6[5] * er[2];
        sum += vx.w * (er[0] * Me0 + er[1] * Me1 + er[2] * Me2);
    }
    return sum;
}

// one source point of update_correspondences + linearize at pose T: v[0..20] H (upper triangle), v[21..26] b, v[27] error;
// the correspondence (voxel slot, Mahalanobis matrix) goes to slot_out / M_out -- DIRECT7 / DIRECT27: the pairs' slots to slot_out, the pose to T_out
template <int kSearch>
__device__ __forceinline__ void vgicp_lin_point(const VgicpArgs& a, const GridHeader& h, const Pose16& T, uint32_t i, double v[28],
                                                uint32_t* __restrict__ slot_out, double* __restrict__ M_out, double* __restrict__ T_out) {
    static_assert(kSearch == PCR_VGICP_DIRECT27 || kSearch == PCR_VGICP_DIRECT7 || kSearch == PCR_VGICP_DIRECT1, "kSearch must be PCR_VGICP_DIRECT27, _DIRECT7 or _DIRECT1");
    if constexpr (kSearch != PCR_VGICP_DIRECT1) { vgicp_lin_pairs<kSearch>(a, h, T, i, v, slot_out, T_out); return; }
    const float* sp = a.src + (size_t)i * a.src_stride;
    const double p[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
    double tp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) tp[r] = T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0;
    uint32_t slot = vgicp_lookup(h, a.cell_start, tp, a.roi);
    if (a.escapes && h.clamped) {
        // The index covers only the bulk of the target (a stray point made its box too large for dense tables).  A source point that
        // lands near -- or beyond -- a face behind which target points were left out would meet voxels whose covariances lack
        // neighbours, or miss a voxel altogether: counted, and the host fails the call instead of returning a pose of the cut map.
        const double c[3] = {floor(tp[0] / h.cell - h.shift) - h.org[0], floor(tp[1] / h.cell - h.shift) - h.org[1], floor(tp[2] / h.cell - h.shift) - h.org[2]};
        const double g = (double)(kPad + a.guard_cells);
        bool esc = false;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            esc = esc || ((h.cut_mask & (1 << d)) && c[d] < g) || ((h.cut_mask & (8 << d)) && c[d] >= (double)h.dims[d] - g);
        if (esc) atomicAdd(a.escapes, 1u);
    }
    if (a.use_tile && !(tp[0] >= a.tile_lo[0] && tp[0] < a.tile_hi[0] && tp[1] >= a.tile_lo[1] && tp[1] < a.tile_hi[1] &&
                        tp[2] >= a.tile_lo[2] && tp[2] < a.tile_hi[2])) slot = 0;      // sharded target: another rank's query
    slot_out[i] = slot;
    if (!slot) return;
    const VgicpVoxel vx = a.vox[slot - 1];
    const double* ca = a.src_cov6 + (size_t)i * 6;
    const double CA[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
    double RC[3][3], S[6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) RC[r][c] = T.m[r] * CA[0][c] + T.m[4 + r] * CA[1][c] + T.m[8 + r] * CA[2][c];
    int o = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) { S[o] = vx.cov[o] + (RC[r][0] * T.m[c] + RC[r][1] * T.m[4 + c] + RC[r][2] * T.m[8 + c]); ++o; }
    double M6[6];
    inv3_sym(S, M6);   // (C_B + T C_A T^T)^-1, fast_vgicp_impl.hpp:104-115
#pragma unroll
    for (int k = 0; k < 6; ++k) M_out[(size_t)i * 6 + k] = M6[k];
    const double M[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
    const double er[3] = {vx.mean[0] - tp[0], vx.mean[1] - tp[1], vx.mean[2] - tp[2]};
    double Me[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Me[r] = M[r][0] * er[0] + M[r][1] * er[1] + M[r][2] * er[2];
    const double w = vx.w;
    // J = [skew(Tp) | -I]   fast_vgicp_impl.hpp:156-158, so3.hpp:21-31
    const double J[3][6] = {{0, -tp[2], tp[1], -1, 0, 0}, {tp[2], 0, -tp[0], 0, -1, 0}, {-tp[1], tp[0], 0, 0, 0, -1}};
    double MJ[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) MJ[r][c] = M[r][0] * J[0][c] + M[r][1] * J[1][c] + M[r][2] * J[2][c];
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[q++] = w * (J[0][r] * MJ[0][c] + J[1][r] * MJ[1][c] + J[2][r] * MJ[2][c]);
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = w * (J[0][r] * Me[0] + J[1][r] * Me[1] + J[2][r] * Me[2]);
    v[27] = w * (er[0] * Me[0] + er[1] * Me[1] + er[2] * Me[2]);
}

// compute_error (fast_vgicp_impl.hpp:183-204) of one point: the correspondences and Mahalanobis matrices of the LAST
// linearisation, new pose
template <int kSearch>
__device__ __forceinline__ double vgicp_err_point(const VgicpArgs& a, const Pose16& T, uint32_t i) {
    if constexpr (kSearch != PCR_VGICP_DIRECT1) return vgicp_err_pairs<kSearch>(a, T, i);
    const uint32_t slot = a.corr_slot[i];
    if (!slot) return 0.0;
    const float* sp = a.src + (size_t)i * a.src_stride;
    const double p[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
    const VgicpVoxel vx = a.vox[slot - 1];
    double er[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) er[r] = vx.mean[r] - (T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0);
    const double* M6 = a.corr_M + (size_t)i * 6;
    const double Me0 = M6[0] * er[0] + M6[1] * er[1] + M6[2] * er[2], Me1 = M6[1] * er[0] + M6[3] * er[1] + M6[4] * er[2],
                 Me2 = M6[2] * er[0] + M6[4] * er[1] + M6[5] * er[2];
    return vx.w * (er[0] * Me0 + er[1] * Me1 + er[2] * Me2);
}

// The pass of lsq_pass.h over VGICP's voxel correspondences: the launch's arguments and the target index header, loaded once
template <int kSearch>
struct VgicpPass {
    const VgicpArgs& a;
    const GridHeader h;
    __device__ __forceinline__ explicit VgicpPass(const VgicpArgs& a_) : a(a_), h(*a_.hdr) {}
    __device__ __forceinline__ void lin(const Pose16& T, uint32_t i, double v[28], bool to_next) const {
        vgicp_lin_point<kSearch>(a, h, T, i, v, to_next ? a.corr_slot_next : a.corr_slot, to_next ? a.corr_M_next : a.corr_M, to_next ? a.corr_T_next : a.corr_T);
    }
    __device__ __forceinline__ double err(const Pose16& T, uint32_t i) const { return vgicp_err_point<kSearch>(a, T, i); }
};

template <bool kWithError, int kSearch>
__global__ __launch_bounds__(256) void vgicp_linearize_kernel(const VgicpArgs a, const Pose16 T) {
    __shared__ double sh[(kWithError ? 29 : 28) * kLinStride];
    __shared__ double sh_sum[8 * 32];
    lsq_lin_body<kWithError>(VgicpPass<kSearch>(a), T, a.n_src, a.partials, sh, sh_sum);
}

// a launch of the device-resident Levenberg-Marquardt loop (lsq_pass.h); roi: a target prepared for one scan reports its escapes with the result
template <int kSearch>
__global__ __launch_bounds__(256) void vgicp_pass_pro_kernel(const VgicpArgs a, const LsqProArgs pa) {
    __shared__ double sh[29 * kLinStride];
    __shared__ double sh_sum[8 * 32];
    __shared__ __attribute__((aligned(16))) uint32_t sh_ctl[kVgCtlWords];
    __shared__ double sh_sums[32];
    lsq_pass<true, VgicpPass<kSearch>>(a, pa, a.roi.mask ? a.roi.escapes : nullptr, sh, sh_sum, sh_ctl, sh_sums);
}

// Sharded targets over the peer exchange (pcr_comm_init_peer): between two passes ONE launch folds this rank's rows of the pass that has just run --
// the order of vgicp_pass_pro_kernel's own fold -- pushes the 32 sums into every peer's receive buffer and folds what arrived in rank order
// (peer_exchange.h); the next pass's prologue takes the result (LsqProArgs::reduced) and the optimiser's step as ever, in every block, on every rank,
// on the same bits.  Two launches per pass and no host round trip, where the host-driven loop of a sharded target has one per pass.  Once the loop
// has finished (the state the pass before left says so, on every rank in the same launch) nothing is exchanged.
__global__ __launch_bounds__(256) void vgicp_peer_exchange_kernel(const double* __restrict__ rows, uint32_t n_rows, const VgCtl* __restrict__ ctl, const PeerComm pc,
                                                                  const double xseq, double* __restrict__ reduced) {
    __shared__ double sh_sum[8 * 32];
    const int t = threadIdx.x, comp = t & 31, slice = t >> 5;
    if (ctl->done) return;
    sh_sum[slice * 32 + comp] = lsq_fold_rows<false>(rows, n_rows, 0, nullptr, nullptr);
    __syncthreads();
    double mine = 0.0;
    if (t < 32) {
        mine = sh_sum[t];
#pragma unroll
        for (int k = 1; k < 8; ++k) mine += sh_sum[k * 32 + t];
    }
    peer_exchange_block(pc, xseq, nullptr, mine, 32, 0, reduced);      // (a rank that never arrives: the status word says so to the host, which ends the call and the session)
}

struct VgCtlArg { uint32_t w[kVgCtlWords]; };
__global__ __launch_bounds__(256) void vgicp_ctl_store_kernel(VgCtl* __restrict__ ctl, const VgCtlArg init, uint32_t* __restrict__ roi_escapes) {
    for (int t = threadIdx.x; t < kVgCtlWords; t += 256) reinterpret_cast<uint32_t*>(ctl)[t] = init.w[t];
    if (roi_escapes && threadIdx.x == 0) *roi_escapes = 0u;
}

// fold per-block partials (32 doubles each) into 32 doubles, fixed order
// out lives in host-mapped memory: out[31] receives `seq` LAST (system-scope release), the word the host spins on
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ partials, uint32_t nblocks, double* __restrict__ out, double seq) {
    __shared__ double sh[8 * 32];
    const int t = threadIdx.x, comp = t & 31, slice = t >> 5;
    double acc = 0.0;
    // eight loads in flight per step, added in the order of a plain loop (same sums, a quarter of the round trips)
    for (uint32_t b0 = slice; b0 < nblocks; b0 += 64) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const uint32_t b = b0 + 8u * u; v[u] = b < nblocks ? partials[(size_t)b * 32 + comp] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (b0 + 8u * u < nblocks) acc += v[u];
    }
    sh[slice * 32 + comp] = acc;
    __syncthreads();
    if (t < 31) {
        double v = sh[t];
#pragma unroll
        for (int s = 1; s < 8; ++s) v += sh[s * 32 + t];
        out[t] = v;
        __threadfence_system();
    }
    __syncthreads();
    if (t == 0) __hip_atomic_store(&out[31], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------
// PCL fitness score: mean squared 1-NN distance of the transformed source
// (pcl::transformPointCloud in float, float kd-tree distances)
// ------------------------------------------------------------------------------
struct PoseF16 { float m[16]; };

__global__ __launch_bounds__(256) void fitness_kernel(GridView g, const float* __restrict__ src, uint32_t n_src, uint32_t stride,
                                                      const PoseF16 T, float max_range, double* __restrict__ partials, const FitTile tile) {
    __shared__ double sh[256];
    __shared__ double shc[256];
    __shared__ double shv[256];
    double acc = 0.0, cnt = 0.0, viol = 0.0;
    // an index cut to a region (header.clamped: the bulk of the cloud, or the room around a scan) holds every target point between the faces of
    // its lattice's interior; beyond a face marked in cut_mask lie points it left out.  Those faces bound the search as a tile's halo does.
    const GridHeader& gh = *g.hdr;
    const int cut = gh.clamped && !gh.empty ? gh.cut_mask : 0;
    double cut_lo[3], cut_hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        cut_lo[d] = (cut >> d) & 1 ? (gh.org[d] + kPad + gh.shift) * gh.cell : -1e300;
        cut_hi[d] = (cut >> (3 + d)) & 1 ? (gh.org[d] + gh.dims[d] - kPad + gh.shift) * gh.cell : 1e300;
    }
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_src; i += gridDim.x * 256) {
        const float* p = src + (size_t)i * stride;
        const float qx = T.m[0] * p[0] + T.m[4] * p[1] + T.m[8] * p[2] + T.m[12];
        const float qy = T.m[1] * p[0] + T.m[5] * p[1] + T.m[9] * p[2] + T.m[13];
        const float qz = T.m[2] * p[0] + T.m[6] * p[1] + T.m[10] * p[2] + T.m[14];
        const double qd[3] = {(double)qx, (double)qy, (double)qz};
        double margin = 1e300;
        if (tile.use) {         // sharded target: the rank whose tile holds the transformed point scores it
            bool in = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                in = in && qd[d] >= tile.lo[d] && qd[d] < tile.hi[d];
                margin = fmin(margin, fmin(qd[d] - tile.ext_lo[d], tile.ext_hi[d] - qd[d]));
            }
            if (!in) continue;
        }
        if (cut && isfinite(qx) && isfinite(qy) && isfinite(qz)) {      // (a point with a coordinate that is not finite is at no finite distance from anything)
#pragma unroll
            for (int d = 0; d < 3; ++d) margin = fmin(margin, fmin(qd[d] - cut_lo[d], cut_hi[d] - qd[d]));
        }
        KeyList<1> L;
        ring_knn<1>(one_level(g), qx, qy, qz, max_range, L);
        float d = 3.0e38f;
        if (L.k[0] != ~0ull) {
            d = __uint_as_float((uint32_t)(L.k[0] >> 32));
            if (d <= max_range) { acc += (double)d; cnt += 1.0; }
        }
        // the nearest point of the rank's cloud (of the cut index) is the map's nearest only if it is nearer than the faces of the region the
        // cloud is complete in (or than the gate: farther points do not count anyway)
        if ((tile.use || cut) && margin < 1e29 && !(sqrt((double)d) * (1.0 + 1e-6) < margin) && !(sqrt((double)max_range) * (1.0 + 1e-6) < margin))
            viol += 1.0;
    }
    sh[threadIdx.x] = acc; shc[threadIdx.x] = cnt; shv[threadIdx.x] = viol;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) { sh[threadIdx.x] += sh[threadIdx.x + s]; shc[threadIdx.x] += shc[threadIdx.x + s]; shv[threadIdx.x] += shv[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[(size_t)blockIdx.x * 32] = sh[0]; partials[(size_t)blockIdx.x * 32 + 1] = shc[0]; partials[(size_t)blockIdx.x * 32 + 2] = shv[0];
        for (int k = 3; k < 32; ++k) partials[(size_t)blockIdx.x * 32 + k] = 0.0;
    }
}

// ---- host launchers ---------------------------------------------------------------
hipError_t vgicp_launch_cov(const GridIndex& grid, const GridIndex* coarse1, const GridIndex* coarse2, const float* d_orig, size_t stride_floats,
                            size_t n, double* d_cov6, hipStream_t s, int reg, const CovCheck* check, const RoiView* roi, CovScratch* scratch, hipEvent_t* ev) {
    if (scratch && n <= 300000 && n > 0) {      // scan-sized: two classes of queries (cov_search.hip)
        const hipError_t e = scratch->reserve(n);
        return e != hipSuccess ? e : cov_search_launch(grid, coarse1, coarse2, d_orig, stride_floats, n, d_cov6, s, check, roi, *scratch, reg, ev);
    }
    const int blocks = (int)std::min<size_t>(65535, (n + 255) / 256 ? (n + 255) / 256 : 1);
    const int levels = coarse1 ? (coarse2 ? 3 : 2) : 1;
    CovCheck chk;
    memset(&chk, 0, sizeof chk);
    if (check) chk = *check;
    RoiView rv;
    memset(&rv, 0, sizeof rv);
    if (roi) rv = *roi;
    // (ev: events stamped at the kernel's own begin and end -- profiling passes)
    // a map-sized target prepared for one scan: the region's points are listed first, and the search runs over the list
    const uint32_t* d_list = nullptr;
    const uint32_t* d_list_count = nullptr;
    int cov_blocks = blocks;
    if (n > 300000 && roi && roi->mask && scratch && !check) {
        const hipError_t e = scratch->reserve_region(n, s);
        if (e != hipSuccess) return e;
        scratch->region_idx ^= 1;
        uint32_t* const cnt = scratch->region_count.as<uint32_t>() + 32 * scratch->region_idx;
        uint32_t* const cnt_next = scratch->region_count.as<uint32_t>() + 32 * (scratch->region_idx ^ 1);
        const int lb = (int)std::min<size_t>(2048, (n + 1023) / 1024);
        hipLaunchKernelGGL(vgicp_region_list_kernel, dim3(lb), dim3(256), 0, s, grid.view(), (uint32_t)n, rv, scratch->region_list.as<uint32_t>(), cnt, cnt_next);
        d_list = scratch->region_list.as<uint32_t>(); d_list_count = cnt;
        cov_blocks = std::min(blocks, 1024);      // (four blocks per CU resident at once; the kernel strides over the list)
    }
#define PCR_COV_ARGS grid.view(), coarse1 ? coarse1->view() : grid.view(), coarse2 ? coarse2->view() : grid.view(), levels, d_orig, (uint32_t)stride_floats, (uint32_t)n, d_cov6, check ? 1 : 0, chk, rv, d_list, d_list_count
    if (n <= 300000) {      // scan-sized (the same threshold as the choice of search levels, vgicp_host.hip: cov_levels)
        COV_REG_DISPATCH(reg, if (ev) hipExtLaunchKernelGGL((vgicp_cov_kernel<true, kReg>), dim3(blocks), dim3(256), 0, s, ev[0], ev[1], 0, PCR_COV_ARGS);
                              else hipLaunchKernelGGL((vgicp_cov_kernel<true, kReg>), dim3(blocks), dim3(256), 0, s, PCR_COV_ARGS))
    } else {
        COV_REG_DISPATCH(reg, if (ev) hipExtLaunchKernelGGL((vgicp_cov_kernel<false, kReg>), dim3(cov_blocks), dim3(256), 0, s, ev[0], ev[1], 0, PCR_COV_ARGS);
                              else hipLaunchKernelGGL((vgicp_cov_kernel<false, kReg>), dim3(cov_blocks), dim3(256), 0, s, PCR_COV_ARGS))
    }
#undef PCR_COV_ARGS
    return hipGetLastError();
}

hipError_t vgicp_launch_voxels(const GridIndex& grid, const double* d_cov6, VgicpVoxel* d_vox, hipStream_t s, int reg, int mode, const RoiView* roi) {
    const size_t n = grid.n_points;
    const int blocks = (int)std::min<size_t>(65535, (n + 255) / 256 ? (n + 255) / 256 : 1);
    RoiView rv;
    memset(&rv, 0, sizeof rv);
    if (roi) rv = *roi;
    // (ADDITIVE_WEIGHTED is ADDITIVE: fast_vgicp_voxel.hpp:138-141)
    if (mode == PCR_VOXEL_MULTIPLICATIVE) hipLaunchKernelGGL(vgicp_voxel_kernel<kFoldMult>, dim3(blocks), dim3(256), 0, s, grid.view(), d_cov6, d_vox, rv);
    else if (reg == PCR_REG_PLANE || reg == PCR_REG_NORMALIZED_MIN_EIG) hipLaunchKernelGGL(vgicp_voxel_kernel<kFoldFixed>, dim3(blocks), dim3(256), 0, s, grid.view(), d_cov6, d_vox, rv);
    else hipLaunchKernelGGL(vgicp_voxel_kernel<kFoldScaled>, dim3(blocks), dim3(256), 0, s, grid.view(), d_cov6, d_vox, rv);
    return hipGetLastError();
}

uint32_t vgicp_blocks(uint32_t n_src) {
    uint32_t b = (n_src + 255) / 256;
    return b < 1 ? 1 : (b > 512 ? 512 : b);
}

// pcr_params.vgicp_search -> the kernel instantiation (VgicpArgs::search; validated by pcr_create / pcr_set_params)
#define VGICP_SEARCH_DISPATCH(search, CALL) \
    switch (search) { \
        case PCR_VGICP_DIRECT27: { constexpr int kSearch = PCR_VGICP_DIRECT27; CALL; } break; \
        case PCR_VGICP_DIRECT7: { constexpr int kSearch = PCR_VGICP_DIRECT7; CALL; } break; \
        case PCR_VGICP_DIRECT1: { constexpr int kSearch = PCR_VGICP_DIRECT1; CALL; } break; \
        default: return hipErrorInvalidValue; \
    }

hipError_t vgicp_launch_linearize(const VgicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq) {
    const uint32_t nb = vgicp_blocks(a.n_src);
    VGICP_SEARCH_DISPATCH(a.search, hipLaunchKernelGGL((vgicp_linearize_kernel<false, kSearch>), dim3(nb), dim3(256), 0, s, a, T))
    return sum_partials_launch(a.partials, nb, d_out32, s, seq);
}

hipError_t vgicp_launch_ctl_init(VgCtl* d_ctl2, const Pose16& guess, int max_iters, int lm_inner, double lm_init_scale, double rot_eps, double trans_eps, hipStream_t s,
                                 uint32_t* d_roi_escapes) {
    VgCtl c;
    memset(&c, 0, sizeof c);
    vg_opt::ctl_init(&c, guess, max_iters, lm_inner, lm_init_scale, rot_eps, trans_eps);
    VgCtlArg arg;
    memcpy(arg.w, &c, sizeof c);
    hipLaunchKernelGGL(vgicp_ctl_store_kernel, dim3(1), dim3(256), 0, s, d_ctl2, arg, d_roi_escapes);
    return hipGetLastError();
}
// launch `index` of the device-resident loop (lsq_pass.h: lsq_pro_args)
// pc / xseq / d_reduced (sharded over the peer exchange, launches after the first): the exchange launch in front of the pass
hipError_t vgicp_launch_pass_pro(const VgicpArgs& a_in, VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, hipStream_t s, double seq, int index,
                                 const PeerComm* pc, double xseq, double* d_reduced) {
    const uint32_t nb = vgicp_blocks(a_in.n_src);
    VgicpArgs a = a_in;
    a.partials = lsq_rows(d_rows2, index);
    LsqProArgs pa = lsq_pro_args(d_ctl2, d_rows2, d_out, seq, index, nb);
    pa.reduced = pc ? d_reduced : nullptr;
    if (pc && index > 0) hipLaunchKernelGGL(vgicp_peer_exchange_kernel, dim3(1), dim3(256), 0, s, pa.rows_prev, nb, pa.ctl_prev, *pc, xseq, d_reduced);
    VGICP_SEARCH_DISPATCH(a.search, hipLaunchKernelGGL(vgicp_pass_pro_kernel<kSearch>, dim3(nb), dim3(256), 0, s, a, pa))
    return hipGetLastError();
}

hipError_t vgicp_launch_error(const VgicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq) {
    const uint32_t nb = vgicp_blocks(a.n_src);
    VGICP_SEARCH_DISPATCH(a.search, hipLaunchKernelGGL((vgicp_linearize_kernel<true, kSearch>), dim3(nb), dim3(256), 0, s, a, T))
    return sum_partials_launch(a.partials, nb, d_out32, s, seq);
}

// (every pass and score that leaves its rows in the [block][32] layout: here and gicp.hip)
hipError_t sum_partials_launch(const double* d_partials, uint32_t nblocks, double* d_out32, hipStream_t s, double seq) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, d_partials, nblocks, d_out32, seq);
    return hipGetLastError();
}

hipError_t fitness_launch(const GridIndex& grid, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16], double max_range,
                          double* d_partials, double* d_out32, hipStream_t s, double seq, const FitTile* tile) {
    PoseF16 T;
    for (int i = 0; i < 16; ++i) T.m[i] = (float)pose[i];
    const uint32_t nb = vgicp_blocks((uint32_t)n_src);
    // the gate is "squared distance <= max_range" in double (PCL: float distances against a double max_range); distances are floats, so
    // the largest float not above max_range is the same gate
    float mr = max_range >= (double)FLT_MAX ? FLT_MAX : (float)max_range;
    if ((double)mr > max_range) mr = nextafterf(mr, -FLT_MAX);
    FitTile ft;
    memset(&ft, 0, sizeof ft);
    if (tile) ft = *tile;
    hipLaunchKernelGGL(fitness_kernel, dim3(nb), dim3(256), 0, s, grid.view(), d_src, (uint32_t)n_src, (uint32_t)stride_floats, T, mr, d_partials, ft);
    return sum_partials_launch(d_partials, nb, d_out32, s, seq);
}

}  // namespace pcr
