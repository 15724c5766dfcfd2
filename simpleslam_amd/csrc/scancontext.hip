// scancontext.hip -- the loop-closure descriptor of the reference's back end:
//   backend/src/ScanContext.cpp (adapted there from irapkaist/scancontext), backend/include/backend/ScanContext.hpp
// makeScanContext (:151-196) -- the per-point part: polar binning of a down-sampled scan into 20 rings x 60 sectors over
// 80 m, maximum of z + lidar_height per bin -- is a device kernel (float atomic max: order-independent, so the
// descriptor is bit-identical to a sequential evaluation).  Everything after it works on 20 x 60 doubles per key frame
// and stays host C++, restated line by line: ring key / sector key (:198-229), fastAlignUsingVkey (:94-114),
// distanceBtnScanContext (:116-150), computeSimularity (:68-92), query with its lazily rebuilt candidate tree (:231-279;
// an exact 10-NN over the 20-dimensional ring keys, by brute force here instead of nanoflann's VectorOfVectorsKdTree).
// Every descriptor is also kept in HBM (float, 4 800 B per context) for pcr_sc_distances: distanceBtnScanContext of an outside scan
// against EVERY stored context, one wave per context (sc_rank_kernel), each sum in the host's order so that the result is the host's bit for bit.
// pcr_sc_rank_stored does the same for stored queries against stored candidates -- lcHandler's walk over a range of key frames
// (LoopClosureManager.cpp:73) -- in tiles of 8 queries x 128 candidates (sc_rank_stored_kernel), the k best per query merged in a fixed order.
// pcr_sc_add_keyframes fills the database from a range of a key-frame store's key frames in one batched pass (sc_polar_batch_kernel).
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/pcr_hip.h"

namespace {

constexpr int kRings = 20, kSectors = 60;            // ScanContext.hpp:17-18
constexpr float kMaxRadius = 80.0f;                  // ScanContext.hpp:19
constexpr float kNoPoint = -1000.0f;                 // ScanContext.cpp:157

// atan2f as glibc computes it.  xy2theta (ScanContext.cpp:28-33) calls std::atan2 on floats, i.e. the C library's atan2f, and a point
// whose azimuth is within an ulp of a sector edge changes bins with the last bit of that result.  glibc's atan2f (2.31 ... 2.35, the
// releases under the reference's ROS targets) is the fdlibm routine in plain float arithmetic -- it is NOT correctly rounded (16 % of
// arguments differ from the rounded double atan2), so the device's own libm cannot stand in for it.  The routine below is that
// published algorithm (Sun fdlibm e_atan2f / s_atanf: argument reduction against atan(0.5), atan(1), atan(1.5), atan(inf) with
// split constants, an odd polynomial of degree 21); built without FMA contraction it reproduced this image's glibc bit for bit on
// 20.4 million arguments (a 1/4 m lattice and random points).  Only IEEE float +, -, *, / are involved, which the GPU rounds identically.
__host__ __device__ inline float sc_atanf(float x) {
    const float atanhi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
    const float atanlo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
    const float aT[11] = {3.3333334327e-01f, -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f, 9.0908870101e-02f, -7.6918758452e-02f,
                          6.6610731184e-02f, -5.8335702866e-02f, 4.9768779427e-02f, -3.6531571299e-02f, 1.6285819933e-02f};
    union { float f; int i; } u;
    u.f = x;
    const int hx = u.i, ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c800000) {                      // |x| >= 2^26
        if (ix > 0x7f800000) return x + x;       // NaN
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {                       // |x| < 0.4375
        if (ix < 0x31000000 && 1.0e30f + x > 1.0f) return x;
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {                   // |x| < 1.1875
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
        else { id = 3; x = -1.0f / x; }
    }
    float z = x * x;
    const float w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    z = (id == 0 ? atanhi[0] : id == 1 ? atanhi[1] : id == 2 ? atanhi[2] : atanhi[3]) -
        ((x * (s1 + s2) - (id == 0 ? atanlo[0] : id == 1 ? atanlo[1] : id == 2 ? atanlo[2] : atanlo[3])) - x);
    return hx < 0 ? -z : z;
}
__host__ __device__ inline float sc_atan2f(float y, float x) {
    const float pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f, tiny = 1.0e-30f;
    union { float f; int i; } ux, uy;
    ux.f = x; uy.f = y;
    const int hx = ux.i, ix = hx & 0x7fffffff, hy = uy.i, iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return sc_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny;
        return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = sc_atanf(fabsf(y / x));
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

// bin of one point, arithmetic type for type as the reference writes it (ScanContext.cpp:27-32,163-181)
__host__ __device__ inline bool sc_bin(float x, float y, int* ring, int* sector) {
    const float azim_range = sqrtf(x * x + y * y);
    float res = (float)((double)sc_atan2f(y, x) + 3.14159265358979323846);       // xy2theta: float atan2 (the C library's: above) + M_PI, stored as float
    res = fmaxf(0.0f, fminf((float)(2 * 3.14159265358979323846), res));
    const float azim_angle = (float)((double)res * 180.0 / 3.14159265358979323846);   // trans::rad2deg<float>
    if (azim_range > kMaxRadius) return false;
    const int r = (int)ceilf((azim_range / kMaxRadius) * kRings);
    const int s = (int)ceil(((double)azim_angle / 360.0) * kSectors);
    *ring = max(min(kRings, r), 1) - 1;
    *sector = max(min(kSectors, s), 1) - 1;
    return true;
}

__global__ __launch_bounds__(256) void sc_polar_kernel(const float* __restrict__ pts, unsigned int n, unsigned int stride, float lidar_height,
                                                       float* __restrict__ desc /* [ring][sector], preset to kNoPoint */) {
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float* p = pts + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2] + lidar_height;
        int ring, sector;
        if (!(isfinite(x) && isfinite(y) && z == z)) continue;   // the reference's int(ceil(NaN)) is undefined behaviour; a NaN z never wins its '<'
        if (!sc_bin(x, y, &ring, &sector)) continue;
        atomicMax(&desc[ring * kSectors + sector], z);
    }
}

// ---- a range of stored key frames in one pass: pcr_sc_add_keyframes ----
// LoopClosureManager::addContext (LoopClosureManager.cpp:28-37) walks the new key frames and bins each one's own cloud; here the walk is one launch.
// Key frame f of the table has n points from float `off` behind pts and owns row f of `rows`.  A block bins one slab of kScSlab points of one
// key frame (jobs[blockIdx.x]: the key frame and the slab's first point) into a descriptor in LDS -- sc_bin and the tests of sc_polar_kernel,
// float max by LDS atomic -- and writes it out along the row: with plain stores when the key frame is that one slab (an empty key frame's one
// block writes the empty row), else by the float atomic max of sc_polar_kernel onto a row preset to kNoPoint (sc_fill_kernel), bins the slab
// left empty skipped.  The maximum of a set of floats does not depend on how the set is cut, so every row holds the bits sc_polar_kernel leaves.
constexpr unsigned int kScSlab = 4096;
struct ScKf { unsigned long long off; unsigned int n, pad_; };
struct ScJob { unsigned int kf, start; };

__global__ __launch_bounds__(256) void sc_fill_kernel(float* __restrict__ p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

__global__ __launch_bounds__(256) void sc_polar_batch_kernel(const float* __restrict__ pts, const ScKf* __restrict__ kfs, const ScJob* __restrict__ jobs,
                                                             unsigned int stride, float lidar_height, float* __restrict__ rows) {
    __shared__ float s_desc[kRings * kSectors];
    const ScJob job = jobs[blockIdx.x];
    const ScKf kf = kfs[job.kf];
    for (int i = threadIdx.x; i < kRings * kSectors; i += 256) s_desc[i] = kNoPoint;
    __syncthreads();
    const unsigned int len = kf.n - job.start < kScSlab ? kf.n - job.start : kScSlab;      // (job.start < kf.n, or both 0)
    const float* base = pts + kf.off + (size_t)job.start * stride;
    for (unsigned int t = threadIdx.x; t < len; t += 256) {
        const float* p = base + (size_t)t * stride;
        const float x = p[0], y = p[1], z = p[2] + lidar_height;
        int ring, sector;
        if (!(isfinite(x) && isfinite(y) && z == z)) continue;   // as sc_polar_kernel
        if (!sc_bin(x, y, &ring, &sector)) continue;
        atomicMax(&s_desc[ring * kSectors + sector], z);
    }
    __syncthreads();
    float* row = rows + (size_t)job.kf * (kRings * kSectors);
    if (kf.n <= kScSlab) {
        for (int i = threadIdx.x; i < kRings * kSectors; i += 256) row[i] = s_desc[i];
    } else {
        for (int i = threadIdx.x; i < kRings * kSectors; i += 256) { const float v = s_desc[i]; if (v != kNoPoint) atomicMax(&row[i], v); }
    }
}

// Column norms (sqrt of the r = 0..19 sum of squares) and sector key (r = 0..19 sum, / 20) of the descriptor(s) at q, in the order pcr_sc_add
// and sc_distance take them on the host.  Per descriptor keys[0, 60): norms, [60, 120): sector key.  One block of 64 per descriptor
// (pcr_sc_distances: the one query; pcr_sc_rank_stored: a run of stored contexts).
__global__ __launch_bounds__(64) void sc_query_keys_kernel(const float* __restrict__ q /* [ring][sector], kNoPoint = empty */, double* __restrict__ keys) {
    const int c = threadIdx.x;
    if (c >= kSectors) return;
    q += (size_t)blockIdx.x * (kRings * kSectors);
    keys += (size_t)blockIdx.x * (2 * kSectors);
    double nrm = 0, sum = 0;
    for (int r = 0; r < kRings; ++r) {
        const float v = q[r * kSectors + c];
        const double x = v == kNoPoint ? 0.0 : (double)v;
        nrm += x * x;
        sum += x;
    }
    keys[c] = sqrt(nrm);
    keys[kSectors + c] = sum / kRings;
}

constexpr int kRankWaves = 4;                        // contexts per block per step: one wave each
constexpr int kShiftGroup = 8;                       // shifts whose 60 cosine terms are staged in LDS at once

struct RankBest { double d; int s; };
// (d, s) lexicographic minimum, NaN never winning: the strict '<' of distanceBtnScanContext over ascending shifts
__device__ inline RankBest rank_min(RankBest a, RankBest b) { return (b.d < a.d || (b.d == a.d && b.s < a.s)) ? b : a; }
__device__ inline RankBest wave_rank_min(RankBest v) {
    for (int o = 32; o > 0; o >>= 1) {
        RankBest w;
        w.d = __shfl_xor(v.d, o, 64);
        w.s = __shfl_xor(v.s, o, 64);
        v = rank_min(v, w);
    }
    return v;
}

// distanceBtnScanContext(query, context) as pcr_sc_distance(q, i) computes it on the host -- the query unshifted, the context shifted -- by ONE
// wave, every wave of the block calling it together (its barriers are block-wide).  The per-pair body of sc_rank_kernel and
// sc_rank_stored_kernel; both descriptors (empty bins as 0), their column norms and sector keys are in LDS, s_term is the wave's own
// kShiftGroup * kSectors doubles:
//   lanes 0..59: the fast-align norm of shift s (sequential c = 0..59 sum, sqrt), then a wave arg-min, the lowest shift winning ties;
//   all lanes: the (shift, column) cosine terms of up to kShiftGroup shifts, each a sequential r = 0..19 dot, staged in s_term;
//   one lane per shift: the sequential col = 0..59 sum with its count of non-empty column pairs, then 1 - sum / eff;
//   the minimum over the shifts by (d, s) with NaN (eff = 0) excluded -- the host's strict '<' over ascending shifts.
// Returns (inf, 1 << 30) in every lane when no shift has a non-empty column pair (sc_pair_result turns that into DBL_MAX / 0).
__device__ inline RankBest sc_pair_wave(const float* s_q, const double* s_qn, const double* s_qk, const float* s_b, const double* s_bn,
                                        const double* s_bk, double* s_term, int lane, int radius, int n_shift) {
    // fastAlignUsingVkey: shift s compares query key c with context key c - s
    RankBest fa{__builtin_inf(), 1 << 30};
    if (lane < kSectors) {
        double s2 = 0;
        for (int c = 0; c < kSectors; ++c) { const int k = c - lane < 0 ? c - lane + kSectors : c - lane; const double d = s_qk[c] - s_bk[k]; s2 += d * d; }
        fa.d = sqrt(s2);
        fa.s = lane;
    }
    const int a0 = wave_rank_min(fa).s;
    // the shifts a0 - radius .. a0 + radius (mod 60; all 60 when that covers the circle): order does not matter to a (d, s) minimum
    RankBest best{__builtin_inf(), 1 << 30};
    for (int g0 = 0; g0 < n_shift; g0 += kShiftGroup) {
        const int gn = n_shift - g0 < kShiftGroup ? n_shift - g0 : kShiftGroup;
        for (int t = lane; t < gn * kSectors; t += 64) {
            const int j = t / kSectors, col = t - j * kSectors;
            const int s = n_shift == kSectors ? g0 + j : ((a0 - radius + g0 + j) % kSectors + kSectors) % kSectors;
            const int sc = col - s < 0 ? col - s + kSectors : col - s;
            double dot = 0;
            for (int r = 0; r < kRings; ++r) dot += (double)s_q[r * kSectors + col] * (double)s_b[r * kSectors + sc];
            const double na = s_qn[col], nb = s_bn[sc];
            s_term[t] = (na == 0 || nb == 0) ? __builtin_nan("") : dot / (na * nb);      // (a term itself is always finite)
        }
        __syncthreads();
        RankBest mine{__builtin_inf(), 1 << 30};
        if (lane < gn) {
            double sum = 0;
            int eff = 0;
            for (int col = 0; col < kSectors; ++col) {
                const double t = s_term[lane * kSectors + col];
                if (t == t) { sum = sum + t; eff = eff + 1; }
            }
            const double d = 1.0 - sum / eff;
            if (d == d) { mine.d = d; mine.s = n_shift == kSectors ? g0 + lane : ((a0 - radius + g0 + lane) % kSectors + kSectors) % kSectors; }
        }
        best = rank_min(best, wave_rank_min(mine));
        __syncthreads();
    }
    return best;
}
// what the host returns for it: DBL_MAX / 0 when no shift had a non-empty column pair
__device__ inline RankBest sc_pair_result(RankBest best) {
    return best.d < __builtin_inf() ? best : RankBest{1.7976931348623157e308, 0};
}

// dist[i], shift[i] = distanceBtnScanContext(query, context i) as pcr_sc_distance(q, i) computes it on the host (sc_pair_wave), for an outside
// query against every stored context.  One wave per context (all waves of a block step together, so the block barriers are uniform);
// lanes 0..59 first take the context's column norms and sector key (sequential r = 0..19 sums).
__global__ __launch_bounds__(256) void sc_rank_kernel(const float* __restrict__ db /* M x [ring][sector] */, unsigned int M,
                                                      const float* __restrict__ q, const double* __restrict__ qkeys, int radius,
                                                      double* __restrict__ dist, int* __restrict__ shift) {
    __shared__ float s_q[kRings * kSectors];
    __shared__ double s_qn[kSectors], s_qk[kSectors];
    __shared__ float4 s_b4[kRankWaves][kRings * kSectors / 4];
    __shared__ double s_bn[kRankWaves][kSectors], s_bk[kRankWaves][kSectors];
    __shared__ double s_term[kRankWaves][kShiftGroup * kSectors];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kRings * kSectors; i += 256) { const float v = q[i]; s_q[i] = v == kNoPoint ? 0.f : v; }
    if (tid < kSectors) { s_qn[tid] = qkeys[tid]; s_qk[tid] = qkeys[kSectors + tid]; }
    const int n_shift = 2 * radius + 1 < kSectors ? 2 * radius + 1 : kSectors;
    const float* s_b = reinterpret_cast<const float*>(s_b4[w]);
    __syncthreads();
    for (unsigned int base = blockIdx.x * kRankWaves; base < M; base += gridDim.x * kRankWaves) {
        const unsigned int ctx = base + w;
        const bool live = ctx < M;
        // the context, empty bins (kNoPoint) as the host's 0.0
        const float4* src4 = reinterpret_cast<const float4*>(db + (size_t)(live ? ctx : 0) * (kRings * kSectors));
        for (int i = lane; i < kRings * kSectors / 4; i += 64) {
            float4 v = live ? src4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            v.x = v.x == kNoPoint ? 0.f : v.x; v.y = v.y == kNoPoint ? 0.f : v.y;
            v.z = v.z == kNoPoint ? 0.f : v.z; v.w = v.w == kNoPoint ? 0.f : v.w;
            s_b4[w][i] = v;
        }
        __syncthreads();
        if (lane < kSectors) {
            double nrm = 0, sum = 0;
            for (int r = 0; r < kRings; ++r) { const double x = (double)s_b[r * kSectors + lane]; nrm += x * x; sum += x; }
            s_bn[w][lane] = sqrt(nrm);
            s_bk[w][lane] = sum / kRings;
        }
        __syncthreads();
        const RankBest best = sc_pair_result(sc_pair_wave(s_q, s_qn, s_qk, s_b, s_bn[w], s_bk[w], s_term[w], lane, radius, n_shift));
        if (live && lane == 0) { dist[ctx] = best.d; shift[ctx] = best.s; }
    }
}

// ---- stored against stored: pcr_sc_rank_stored ----
// For every query q of [first, first + count) the k best candidates i of [0, q - excl) by (dist, i), dist and shift as sc_pair_wave gives them.
// The triangle is cut into tiles of kTileQ queries x kTileC candidates, one block each (blockIdx.x = query tile * nct + candidate tile):
// the block keeps its queries' descriptors, norms and keys in LDS and streams the tile's candidates past them kStoredWaves at a time, one
// per wave, so a staged candidate serves kTileQ pairs; the norms and keys of both sides come from `keys` (sc_query_keys_kernel over the
// store, once per context).  The tile's (dist, shift) land in LDS, then wave j selects query j's k best of the tile -- k rounds, each the
// (dist, i) minimum above the previous round's -- into part[((q - first) * nct + tile) * k + r], tail (DBL_MAX, -1, 0).
// sc_rank_merge_kernel does the same selection over the lists of a query's tiles.  A tile with no pair inside the triangle exits at once.
// No atomics and no dependence on scheduling: every list entry has one writer, and (dist, i) is a total order.
constexpr int kTileQ = 8, kTileC = 128, kStoredWaves = 8;
static_assert(kTileQ <= kStoredWaves && kTileC % kStoredWaves == 0 && kTileC % 64 == 0, "one selecting wave per query, whole steps, whole lanes");

__global__ __launch_bounds__(64 * kStoredWaves) void sc_rank_stored_kernel(const float* __restrict__ db, const double* __restrict__ keys, unsigned int first,
                                                                           unsigned int count, unsigned int nct, int excl, int radius, int k,
                                                                           double* __restrict__ part_d, int* __restrict__ part_i, int* __restrict__ part_s) {
    __shared__ float4 s_q4[kTileQ][kRings * kSectors / 4];
    __shared__ double s_qn[kTileQ][kSectors], s_qk[kTileQ][kSectors];
    __shared__ float4 s_b4[kStoredWaves][kRings * kSectors / 4];
    __shared__ double s_bn[kStoredWaves][kSectors], s_bk[kStoredWaves][kSectors];
    __shared__ double s_term[kStoredWaves][kShiftGroup * kSectors];
    __shared__ double s_rd[kTileQ][kTileC];
    __shared__ int s_rs[kTileQ][kTileC];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned int qt = blockIdx.x / nct, ct = blockIdx.x - qt * nct;
    const unsigned int q0 = first + qt * kTileQ;
    const int nq = (int)(first + count - q0 < (unsigned int)kTileQ ? first + count - q0 : (unsigned int)kTileQ);
    const long long c0 = (long long)ct * kTileC;
    const long long lim_last = (long long)(q0 + nq - 1) - excl;      // candidates of the tile's last query: [0, lim_last)
    if (c0 >= lim_last) return;                                      // the whole tile lies outside the triangle
    const int n_shift = 2 * radius + 1 < kSectors ? 2 * radius + 1 : kSectors;
    auto zero_empty = [](float4 v) {                                 // empty bins (kNoPoint) as the host's 0.0
        v.x = v.x == kNoPoint ? 0.f : v.x; v.y = v.y == kNoPoint ? 0.f : v.y;
        v.z = v.z == kNoPoint ? 0.f : v.z; v.w = v.w == kNoPoint ? 0.f : v.w;
        return v;
    };
    for (int j = w; j < nq; j += kStoredWaves) {
        const float4* src4 = reinterpret_cast<const float4*>(db + (size_t)(q0 + j) * (kRings * kSectors));
        for (int i = lane; i < kRings * kSectors / 4; i += 64) s_q4[j][i] = zero_empty(src4[i]);
        if (lane < kSectors) {
            s_qn[j][lane] = keys[(size_t)(q0 + j) * (2 * kSectors) + lane];
            s_qk[j][lane] = keys[(size_t)(q0 + j) * (2 * kSectors) + kSectors + lane];
        }
    }
    const float* s_b = reinterpret_cast<const float*>(s_b4[w]);
    __syncthreads();
    for (long long c = c0; c < c0 + kTileC && c < lim_last; c += kStoredWaves) {      // (block-uniform)
        const long long ctx = c + w;
        const bool live = ctx < lim_last;                            // lim_last <= the last query's own index: inside the store
        const float4* src4 = reinterpret_cast<const float4*>(db + (size_t)(live ? ctx : 0) * (kRings * kSectors));
        for (int i = lane; i < kRings * kSectors / 4; i += 64) s_b4[w][i] = live ? zero_empty(src4[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < kSectors) {
            s_bn[w][lane] = live ? keys[(size_t)ctx * (2 * kSectors) + lane] : 0.0;
            s_bk[w][lane] = live ? keys[(size_t)ctx * (2 * kSectors) + kSectors + lane] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < nq; ++j) {
            if (c >= (long long)(q0 + j) - excl) continue;           // (block-uniform) none of this step's candidates is one of query j's
            const RankBest best = sc_pair_result(sc_pair_wave(reinterpret_cast<const float*>(s_q4[j]), s_qn[j], s_qk[j], s_b, s_bn[w], s_bk[w],
                                                              s_term[w], lane, radius, n_shift));
            if (lane == 0) { s_rd[j][ctx - c0] = best.d; s_rs[j][ctx - c0] = best.s; }      // (entries past query j's limit are never read)
        }
        // sc_pair_wave ends on a barrier, and a step no query took read nothing: the next step may overwrite s_b4
    }
    __syncthreads();
    if (w >= nq) return;
    const long long lim = (long long)(q0 + w) - excl - c0;           // query w's candidates in this tile: entries [0, lim)
    const int n_in = lim < 0 ? 0 : lim > kTileC ? kTileC : (int)lim;
    const size_t out = ((size_t)(q0 + w - first) * nct + ct) * (size_t)k;
    RankBest prev{-__builtin_inf(), -1};
    for (int r = 0; r < k; ++r) {
        RankBest mine{__builtin_inf(), 1 << 30};
        for (int t = lane; t < n_in; t += 64) {
            const RankBest e{s_rd[w][t], t};
            if (e.d > prev.d || (e.d == prev.d && e.s > prev.s)) mine = rank_min(mine, e);
        }
        const RankBest win = wave_rank_min(mine);
        if (win.s == 1 << 30) {
            if (lane == 0) { part_d[out + r] = 1.7976931348623157e308; part_i[out + r] = -1; part_s[out + r] = 0; }
        } else if (lane == (win.s & 63)) {
            part_d[out + r] = win.d; part_i[out + r] = (int)(c0 + win.s); part_s[out + r] = s_rs[w][win.s];
        }
        prev = win;
    }
}

// The k best of query q = first + row over the lists of its candidate tiles (tile t holds candidates of q while t * kTileC < q - excl), by
// (dist, i) as above; one wave per query.  Rows with no candidate get the tail: idx -1, DBL_MAX, shift 0.
__global__ __launch_bounds__(256) void sc_rank_merge_kernel(const double* __restrict__ part_d, const int* __restrict__ part_i, const int* __restrict__ part_s,
                                                            unsigned int first, unsigned int count, unsigned int nct, int excl, int k,
                                                            long long* __restrict__ idx, double* __restrict__ dist, int* __restrict__ shift) {
    const unsigned int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= count) return;
    const long long lim = (long long)(first + row) - excl;
    const size_t n_in = lim <= 0 ? 0 : (size_t)((lim + kTileC - 1) / kTileC) * (size_t)k;      // entries of the row's lists
    const size_t in = (size_t)row * nct * (size_t)k, out = (size_t)row * (size_t)k;
    RankBest prev{-__builtin_inf(), -1};
    for (int r = 0; r < k; ++r) {
        RankBest mine{__builtin_inf(), 0x7fffffff};
        int at = 0;
        for (size_t t = lane; t < n_in; t += 64) {
            const RankBest e{part_d[in + t], part_i[in + t]};
            if (e.s < 0) continue;                                   // a list's tail
            if ((e.d > prev.d || (e.d == prev.d && e.s > prev.s)) && (e.d < mine.d || (e.d == mine.d && e.s < mine.s))) { mine = e; at = part_s[in + t]; }
        }
        const RankBest win = wave_rank_min(mine);
        if (win.s == 0x7fffffff) {
            if (lane == 0) { dist[out + r] = 1.7976931348623157e308; idx[out + r] = -1; shift[out + r] = 0; }
        } else if (mine.s == win.s) {                                // one lane: a candidate stands in one list
            dist[out + r] = win.d; idx[out + r] = win.s; shift[out + r] = at;
        }
        prev = win;
    }
}

struct Desc { double m[kRings * kSectors]; };        // row-major [ring][sector]

}  // namespace

struct pcr_sc {
    int device = 0;
    pcr_sc_params prm;
    std::vector<Desc> polar;
    std::vector<std::vector<double>> ring, sector;
    size_t tree_size = 0;                                // ring_sub_.size(): contexts visible to the candidate search
    float* d_desc = nullptr;
    float* d_stage = nullptr; size_t stage_cap = 0;
    float* d_db = nullptr; size_t db_cap = 0;            // every context's descriptor as binned (kNoPoint = empty), [context][ring][sector]
    float* d_query = nullptr; double* d_qkeys = nullptr; // pcr_sc_distances: the outside scan's descriptor and its column norms + sector key
    double* d_dist = nullptr; int* d_shift = nullptr; size_t res_cap = 0;
    // pcr_sc_rank_stored: column norms + sector key of contexts [0, keys_n) (120 doubles each; a context never changes once added), the
    // per-tile lists of one chunk of queries, and the merged result
    double* d_keys = nullptr; size_t keys_cap = 0, keys_n = 0;
    void* d_part = nullptr; size_t part_cap = 0;
    void* d_rank = nullptr; size_t rank_cap = 0;
    // pcr_sc_add_keyframes: the key-frame and block tables of one call; with a grid_size, the filter (a handle of its own, made by the first
    // such call) and the filtered key frames packed one behind the other
    void* d_tab = nullptr; size_t tab_cap = 0;
    pcr_handle* filter = nullptr;
    void* d_pack = nullptr; size_t pack_cap = 0;
    std::string err;
};

namespace pcr {
int sc_device(const pcr_sc* sc) { return sc->device; }      // (pcr_internal.h)
int map_device(const pcr_map* m);                           // (submap.hip)
}
// (library-internal, voxel_host.hip) the voxel filter in two halves, device memory into device memory: what pcr_map_downsample_keyframes runs per key frame
int pcr_internal_vf_begin(pcr_handle* h, const void* d_pts, size_t n, size_t stride_bytes, double leaf, void* d_out, size_t out_capacity);
int pcr_internal_vf_end(pcr_handle* h, size_t* n_out);

static thread_local std::string g_sc_err;
static int scfail(pcr_sc* s, const std::string& m) { if (s) s->err = m; else g_sc_err = m; return 1; }
#define S_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return scfail(sc, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

namespace {

double col_norm(const Desc& d, int col) { double s = 0; for (int r = 0; r < kRings; ++r) s += d.m[r * kSectors + col] * d.m[r * kSectors + col]; return sqrt(s); }

// computeSimularity of sc1 and sc2 circularly shifted by `shift` columns to the right (ScanContext.cpp:34-54,68-92)
double sc_distance(const Desc& a, const Desc& b, int shift) {
    int eff = 0;
    double sum = 0;
    for (int col = 0; col < kSectors; ++col) {
        const int src = ((col - shift) % kSectors + kSectors) % kSectors;      // shifted(col) = b(col - shift)
        double na = 0, nb = 0, dot = 0;
        for (int r = 0; r < kRings; ++r) {
            const double x = a.m[r * kSectors + col], y = b.m[r * kSectors + src];
            na += x * x; nb += y * y; dot += x * y;
        }
        na = sqrt(na); nb = sqrt(nb);
        if (na == 0 || nb == 0) continue;
        sum = sum + dot / (na * nb);
        eff = eff + 1;
    }
    return 1.0 - sum / eff;                              // eff == 0 gives NaN, as in the reference
}

int fast_align(const std::vector<double>& k1, const std::vector<double>& k2) {        // :94-114 (keys as 1 x 60 rows)
    int arg = 0;
    double best = std::numeric_limits<double>::max();
    for (int shift = 0; shift < kSectors; ++shift) {
        double s = 0;
        for (int c = 0; c < kSectors; ++c) { const double d = k1[c] - k2[((c - shift) % kSectors + kSectors) % kSectors]; s += d * d; }
        const double nrm = sqrt(s);
        if (nrm < best) { arg = shift; best = nrm; }
    }
    return arg;
}

}  // namespace

extern "C" {

void pcr_sc_default_params(pcr_sc_params* p) {
    if (!p) return;
    p->lidar_height = 2.0;            /* config/params.json: tf.lidar_height */
    p->num_exclude_recent = 40;       /* backend.context.scancontext.* */
    p->build_tree_gap = 10;
    p->num_candidates = 10;
    p->search_ratio = 0.1;
    p->dist_thres = 0.4;
}

pcr_sc* pcr_sc_create(int device, const pcr_sc_params* p) {
    pcr_sc* sc = new pcr_sc;
    if (p) sc->prm = *p; else pcr_sc_default_params(&sc->prm);
    if (device >= 0) sc->device = device; else (void)hipGetDevice(&sc->device);
    if (hipSetDevice(sc->device) != hipSuccess || hipMalloc((void**)&sc->d_desc, kRings * kSectors * sizeof(float)) != hipSuccess) {
        g_sc_err = "pcr_sc_create: no usable HIP device (there is no CPU fallback)";
        delete sc;
        return nullptr;
    }
    return sc;
}

void pcr_sc_destroy(pcr_sc* sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->device);
    for (void* p : {(void*)sc->d_desc, (void*)sc->d_stage, (void*)sc->d_db, (void*)sc->d_query, (void*)sc->d_qkeys, (void*)sc->d_dist, (void*)sc->d_shift,
                    (void*)sc->d_keys, sc->d_part, sc->d_rank, sc->d_tab, sc->d_pack})
        if (p) (void)hipFree(p);
    if (sc->filter) pcr_destroy(sc->filter);
    delete sc;
}

const char* pcr_sc_last_error(const pcr_sc* sc) { return sc ? sc->err.c_str() : g_sc_err.c_str(); }

int pcr_sc_size(const pcr_sc* sc, size_t* n) { if (!sc || !n) return 1; *n = sc->polar.size(); return 0; }

}  // extern "C"

namespace {

// The argument checks of pcr_sc_add / pcr_sc_distances, then the polar binning of the cloud into `desc` (1200 floats, preset to kNoPoint).
int sc_bin_cloud(pcr_sc* sc, const void* pts, size_t n, size_t stride_bytes, int on_device, float* desc) {
    if (n && !pts) return scfail(sc, "NULL cloud with nonzero size");
    if (stride_bytes < 12 || stride_bytes % 4) return scfail(sc, "stride_bytes must be a multiple of 4 and >= 12");
    if (n > 0xfffffff0ull) return scfail(sc, "cloud too large");
    S_TRY(hipSetDevice(sc->device));
    const float* d_pts = static_cast<const float*>(pts);
    if (!on_device && n) {
        const size_t bytes = n * stride_bytes;
        if (bytes > sc->stage_cap) {
            if (sc->d_stage) (void)hipFree(sc->d_stage);
            sc->d_stage = nullptr; sc->stage_cap = 0;
            S_TRY(hipMalloc((void**)&sc->d_stage, bytes + bytes / 2));
            sc->stage_cap = bytes + bytes / 2;
        }
        S_TRY(hipMemcpy(sc->d_stage, pts, bytes, hipMemcpyHostToDevice));
        d_pts = sc->d_stage;
    }
    float init[kRings * kSectors];
    for (float& v : init) v = kNoPoint;
    S_TRY(hipMemcpy(desc, init, sizeof init, hipMemcpyHostToDevice));
    if (n) {
        const int blocks = (int)std::min<size_t>(1024, (n + 255) / 256);
        hipLaunchKernelGGL(sc_polar_kernel, dim3(blocks), dim3(256), 0, 0, d_pts, (unsigned int)n, (unsigned int)(stride_bytes / 4),
                           (float)sc->prm.lidar_height, desc);
        S_TRY(hipGetLastError());
    }
    return 0;
}

// Room in the device store for one more context: the store doubles (at least 64 contexts); a failed growth leaves it as it was.
int sc_reserve_one(pcr_sc* sc) {
    const size_t n = sc->polar.size();
    if (n < sc->db_cap) return 0;
    const size_t cap = std::max<size_t>(64, 2 * sc->db_cap);
    const size_t per = (size_t)kRings * kSectors * sizeof(float);
    float* p = nullptr;
    const hipError_t e = hipMalloc((void**)&p, cap * per);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return scfail(sc, "the device store of " + std::to_string(n) + " contexts cannot grow to " + std::to_string(cap) + ": " + hipGetErrorString(e));
    }
    if (n) {
        const hipError_t c = hipMemcpy(p, sc->d_db, n * per, hipMemcpyDeviceToDevice);
        if (c != hipSuccess) { (void)hipFree(p); return scfail(sc, std::string("growing the device store: ") + hipGetErrorString(c)); }
    }
    if (sc->d_db) (void)hipFree(sc->d_db);
    sc->d_db = p; sc->db_cap = cap;
    return 0;
}

// What the host keeps of one binned row (1200 floats): the descriptor with empty bins as 0.0 (:186-190), ring key and sector key (:198-229),
// each a sequential double sum in index order
void sc_host_entry(const float* row, Desc& d, std::vector<double>& rk, std::vector<double>& sk) {
    for (int i = 0; i < kRings * kSectors; ++i) d.m[i] = row[i] == kNoPoint ? 0.0 : (double)row[i];
    for (int r = 0; r < kRings; ++r) { double s = 0; for (int c = 0; c < kSectors; ++c) s += d.m[r * kSectors + c]; rk[r] = s / kSectors; }
    for (int c = 0; c < kSectors; ++c) { double s = 0; for (int r = 0; r < kRings; ++r) s += d.m[r * kSectors + c]; sk[c] = s / kRings; }
}

// Room for `more` contexts behind the stored ones: the capacity the doubling above arrives at, reached with one allocation and one copy.
int sc_reserve_more(pcr_sc* sc, size_t more) {
    const size_t n = sc->polar.size(), per = (size_t)kRings * kSectors * sizeof(float);
    if (more > std::numeric_limits<size_t>::max() / (4 * per) - n) return scfail(sc, "too many contexts");
    if (n + more <= sc->db_cap) return 0;
    size_t cap = sc->db_cap;
    while (cap < n + more) cap = std::max<size_t>(64, 2 * cap);
    float* p = nullptr;
    const hipError_t e = hipMalloc((void**)&p, cap * per);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return scfail(sc, "the device store of " + std::to_string(n) + " contexts cannot grow to " + std::to_string(cap) + ": " + hipGetErrorString(e));
    }
    if (n) {
        const hipError_t c = hipMemcpy(p, sc->d_db, n * per, hipMemcpyDeviceToDevice);
        if (c != hipSuccess) { (void)hipFree(p); return scfail(sc, std::string("growing the device store: ") + hipGetErrorString(c)); }
    }
    if (sc->d_db) (void)hipFree(sc->d_db);
    sc->d_db = p; sc->db_cap = cap;
    return 0;
}

}  // namespace

extern "C" {

/* addContext (:56-66): descriptor of a (down-sampled) scan in the lidar frame + its ring and sector keys */
int pcr_sc_add(pcr_sc* sc, const void* pts, size_t n, size_t stride_bytes, int on_device) {
    if (!sc) return 1;
    sc->err.clear();
    if (sc_bin_cloud(sc, pts, n, stride_bytes, on_device, sc->d_desc)) return 1;
    if (sc_reserve_one(sc)) return 1;
    S_TRY(hipMemcpy(sc->d_db + sc->polar.size() * (kRings * kSectors), sc->d_desc, kRings * kSectors * sizeof(float), hipMemcpyDeviceToDevice));
    float host[kRings * kSectors];
    S_TRY(hipMemcpy(host, sc->d_desc, sizeof host, hipMemcpyDeviceToHost));
    Desc d;
    std::vector<double> rk(kRings), sk(kSectors);
    sc_host_entry(host, d, rk, sk);
    sc->polar.push_back(d); sc->ring.push_back(rk); sc->sector.push_back(sk);
    return 0;
}

int pcr_sc_descriptor(const pcr_sc* sc, size_t id, double* desc_row_major_20x60, double* ring_key_20, double* sector_key_60) {
    if (!sc || id >= sc->polar.size()) return 1;
    if (desc_row_major_20x60) std::copy(sc->polar[id].m, sc->polar[id].m + kRings * kSectors, desc_row_major_20x60);
    if (ring_key_20) std::copy(sc->ring[id].begin(), sc->ring[id].end(), ring_key_20);
    if (sector_key_60) std::copy(sc->sector[id].begin(), sc->sector[id].end(), sector_key_60);
    return 0;
}

/* distanceBtnScanContext (:116-150): minimum over the shifts around the sector-key alignment */
int pcr_sc_distance(const pcr_sc* sc, size_t id1, size_t id2, double* dist, int* shift) {
    if (!sc || id1 >= sc->polar.size() || id2 >= sc->polar.size()) return 1;
    const int a0 = fast_align(sc->sector[id1], sc->sector[id2]);
    const int radius = (int)round(0.5 * (double)(float)sc->prm.search_ratio * kSectors);
    std::vector<int> space{a0};
    for (int ii = 1; ii < radius + 1; ++ii) { space.push_back((a0 + ii + kSectors) % kSectors); space.push_back((a0 - ii + kSectors) % kSectors); }
    std::sort(space.begin(), space.end());
    int arg = 0;
    double best = std::numeric_limits<double>::max();
    for (int s : space) {
        const double d = sc_distance(sc->polar[id1], sc->polar[id2], s);
        if (d < best) { arg = s; best = d; }
    }
    if (dist) *dist = best;
    if (shift) *shift = arg;
    return 0;
}

/* distanceBtnScanContext of an outside scan against every stored context, on the device (sc_rank_kernel) */
int pcr_sc_distances(pcr_sc* sc, const void* pts, size_t n, size_t stride_bytes, int on_device, double* dist, int32_t* shift) {
    if (!sc) return 1;
    sc->err.clear();
    const size_t M = sc->polar.size();
    if (M && (!dist || !shift)) return scfail(sc, "dist or shift is NULL");
    if (M > 0xffffffffull - kRankWaves) return scfail(sc, "too many contexts");
    S_TRY(hipSetDevice(sc->device));
    if (!sc->d_query) {
        S_TRY(hipMalloc((void**)&sc->d_query, kRings * kSectors * sizeof(float)));
        S_TRY(hipMalloc((void**)&sc->d_qkeys, 2 * kSectors * sizeof(double)));
    }
    if (sc_bin_cloud(sc, pts, n, stride_bytes, on_device, sc->d_query)) return 1;
    if (M == 0) return 0;
    if (M > sc->res_cap) {
        if (sc->d_dist) (void)hipFree(sc->d_dist);
        if (sc->d_shift) (void)hipFree(sc->d_shift);
        sc->d_dist = nullptr; sc->d_shift = nullptr; sc->res_cap = 0;
        S_TRY(hipMalloc((void**)&sc->d_dist, sc->db_cap * sizeof(double)));
        S_TRY(hipMalloc((void**)&sc->d_shift, sc->db_cap * sizeof(int)));
        sc->res_cap = sc->db_cap;
    }
    const int radius = std::max(0, (int)round(0.5 * (double)(float)sc->prm.search_ratio * kSectors));      // as pcr_sc_distance
    hipLaunchKernelGGL(sc_query_keys_kernel, dim3(1), dim3(64), 0, 0, sc->d_query, sc->d_qkeys);
    S_TRY(hipGetLastError());
    const unsigned int blocks = (unsigned int)std::min<size_t>((M + kRankWaves - 1) / kRankWaves, 8192);
    hipLaunchKernelGGL(sc_rank_kernel, dim3(blocks), dim3(256), 0, 0, sc->d_db, (unsigned int)M, sc->d_query, sc->d_qkeys, std::min(radius, kSectors),
                       sc->d_dist, sc->d_shift);
    S_TRY(hipGetLastError());
    S_TRY(hipMemcpy(dist, sc->d_dist, M * sizeof(double), hipMemcpyDeviceToHost));
    S_TRY(hipMemcpy(shift, sc->d_shift, M * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

namespace {

// a device buffer of at least `bytes` (contents not kept); a failed growth leaves none
int sc_room(pcr_sc* sc, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    S_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return 0;
}

// column norms and sector keys of contexts [0, n) in d_keys: only those added since the last call are computed
int sc_keys_upto(pcr_sc* sc, size_t n) {
    if (n > sc->keys_cap) {
        double* p = nullptr;
        S_TRY(hipMalloc((void**)&p, sc->db_cap * 2 * kSectors * sizeof(double)));
        if (sc->keys_n) {
            const hipError_t c = hipMemcpy(p, sc->d_keys, sc->keys_n * 2 * kSectors * sizeof(double), hipMemcpyDeviceToDevice);
            if (c != hipSuccess) { (void)hipFree(p); return scfail(sc, std::string("growing the key store: ") + hipGetErrorString(c)); }
        }
        if (sc->d_keys) (void)hipFree(sc->d_keys);
        sc->d_keys = p; sc->keys_cap = sc->db_cap;
    }
    if (n > sc->keys_n) {
        hipLaunchKernelGGL(sc_query_keys_kernel, dim3((unsigned int)(n - sc->keys_n)), dim3(64), 0, 0, sc->d_db + sc->keys_n * (kRings * kSectors),
                           sc->d_keys + sc->keys_n * 2 * kSectors);
        S_TRY(hipGetLastError());
        sc->keys_n = n;
    }
    return 0;
}

}  // namespace

extern "C" {

/* LoopClosureManager::addContext (LoopClosureManager.cpp:28-37) over key frames [first, first + count) of a key-frame store: every stage once for the
 * range -- one table up, one binning launch (sc_polar_batch_kernel) into the rows of the device store, one copy of those rows back, keys on the host
 * as pcr_sc_add takes them.  With a grid_size the key frames first pass the voxel filter one by one (its centroids depend on its own summation order:
 * voxel_filter.hip) into one packed buffer, which is then binned the same way. */
int pcr_sc_add_keyframes(pcr_sc* sc, const pcr_map* m, size_t first, size_t count, double grid_size, size_t* n_added) {
    if (!sc) return scfail(nullptr, "pcr_sc_add_keyframes: sc is NULL");
    sc->err.clear();
    if (!m) return scfail(sc, "pcr_sc_add_keyframes: map is NULL");
    size_t n_kf = 0;
    if (pcr_map_keyframes(m, &n_kf)) return scfail(sc, std::string("pcr_sc_add_keyframes: ") + pcr_map_last_error(m));
    if (first > n_kf || count > n_kf - first)
        return scfail(sc, "pcr_sc_add_keyframes: first + count = " + std::to_string(first) + " + " + std::to_string(count) + " exceeds the " + std::to_string(n_kf) + " key frames");
    if (pcr::map_device(m) != sc->device)
        return scfail(sc, "pcr_sc_add_keyframes: the map is on device " + std::to_string(pcr::map_device(m)) + ", the database on device " + std::to_string(sc->device));
    if (count == 0) { if (n_added) *n_added = 0; return 0; }
    if (count > 0x7fffff00ull) return scfail(sc, "too many key frames in one call");
    S_TRY(hipSetDevice(sc->device));
    const size_t n0 = sc->polar.size(), per = (size_t)kRings * kSectors;
    try {
        // the key frames as pcr_map_keyframe hands them out
        std::vector<const float*> src(count);
        std::vector<size_t> src_n(count);
        size_t stride = 0, total = 0;
        for (size_t i = 0; i < count; ++i) {
            src[i] = static_cast<const float*>(pcr_map_keyframe(m, first + i, &src_n[i], &stride, nullptr));
            if (!src[i] && src_n[i]) return scfail(sc, std::string("pcr_sc_add_keyframes: ") + pcr_map_last_error(m));
            if (src_n[i] > 0xfffffff0ull) return scfail(sc, "cloud too large");
            total += src_n[i];
        }
        if (stride < 12 || stride % 4) return scfail(sc, "stride_bytes must be a multiple of 4 and >= 12");
        const size_t sf = stride / 4;
        std::vector<ScKf> kfs(count);
        const float* base = nullptr;
        if (grid_size > 0 && total) {
            // every key frame through the filter, one behind the other (room for the unfiltered sizes: a grid too fine for a key frame returns it as it is)
            if (!sc->filter) {
                pcr_params p;
                pcr_default_params(&p);
                p.device = sc->device;
                sc->filter = pcr_create("loam", &p);
                if (!sc->filter) return scfail(sc, std::string("pcr_sc_add_keyframes: ") + pcr_last_error(nullptr));
            }
            if (sc_room(sc, &sc->d_pack, &sc->pack_cap, total * stride)) return 1;
            float* pack = static_cast<float*>(sc->d_pack);
            size_t w = 0;
            for (size_t i = 0; i < count; ++i) {
                size_t n_out = 0;
                if (src_n[i] && (pcr_internal_vf_begin(sc->filter, src[i], src_n[i], stride, grid_size, pack + w * sf, src_n[i]) || pcr_internal_vf_end(sc->filter, &n_out)))
                    return scfail(sc, std::string("voxel filter: ") + pcr_last_error(sc->filter));
                kfs[i] = ScKf{(unsigned long long)(w * sf), (unsigned int)n_out, 0};
                w += n_out;
            }
            base = pack;
        } else {
            for (size_t i = 0; i < count; ++i) if (src[i] && (!base || src[i] < base)) base = src[i];
            for (size_t i = 0; i < count; ++i) kfs[i] = ScKf{src[i] ? (unsigned long long)(src[i] - base) : 0ull, (unsigned int)src_n[i], 0};
        }
        // a block per slab, at least one per key frame
        std::vector<ScJob> jobs;
        jobs.reserve(count);
        bool shared_rows = false;
        for (size_t i = 0; i < count; ++i) {
            jobs.push_back(ScJob{(unsigned int)i, 0});
            for (size_t s = kScSlab; s < kfs[i].n; s += kScSlab) jobs.push_back(ScJob{(unsigned int)i, (unsigned int)s});
            shared_rows |= kfs[i].n > kScSlab;
        }
        if (jobs.size() > 0x7fffffffull) return scfail(sc, "too many points in one call");
        const size_t kf_bytes = count * sizeof(ScKf), job_bytes = jobs.size() * sizeof(ScJob);
        if (sc_room(sc, &sc->d_tab, &sc->tab_cap, kf_bytes + job_bytes)) return 1;
        std::vector<char> tab(kf_bytes + job_bytes);
        std::copy(reinterpret_cast<const char*>(kfs.data()), reinterpret_cast<const char*>(kfs.data()) + kf_bytes, tab.begin());
        std::copy(reinterpret_cast<const char*>(jobs.data()), reinterpret_cast<const char*>(jobs.data()) + job_bytes, tab.begin() + kf_bytes);
        std::vector<float> host(count * per);
        sc->polar.reserve(n0 + count); sc->ring.reserve(n0 + count); sc->sector.reserve(n0 + count);
        S_TRY(hipMemcpy(sc->d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
        if (sc_reserve_more(sc, count)) return 1;
        float* rows = sc->d_db + n0 * per;
        if (shared_rows) {
            hipLaunchKernelGGL(sc_fill_kernel, dim3((unsigned int)std::min<size_t>((count * per + 255) / 256, 4096)), dim3(256), 0, 0, rows, count * per, kNoPoint);
            S_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(sc_polar_batch_kernel, dim3((unsigned int)jobs.size()), dim3(256), 0, 0, base, static_cast<const ScKf*>(sc->d_tab),
                           reinterpret_cast<const ScJob*>(static_cast<const char*>(sc->d_tab) + kf_bytes), (unsigned int)sf, (float)sc->prm.lidar_height, rows);
        S_TRY(hipGetLastError());
        S_TRY(hipMemcpy(host.data(), rows, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        try {
            std::vector<double> rk(kRings), sk(kSectors);
            for (size_t i = 0; i < count; ++i) {
                sc->polar.emplace_back();
                sc_host_entry(host.data() + i * per, sc->polar.back(), rk, sk);
                sc->ring.push_back(rk); sc->sector.push_back(sk);
            }
        } catch (const std::bad_alloc&) {
            sc->polar.resize(n0); sc->ring.resize(n0); sc->sector.resize(n0);
            throw;
        }
    } catch (const std::bad_alloc&) {
        return scfail(sc, "pcr_sc_add_keyframes: out of host memory");
    }
    if (n_added) *n_added = count;
    return 0;
}

/* distanceBtnScanContext of stored queries [first, first + count) against every older stored context, the k best each (sc_rank_stored_kernel) */
int pcr_sc_rank_stored(pcr_sc* sc, size_t first, size_t count, int k, int64_t* idx, double* dist, int32_t* shift) {
    if (!sc) return 1;
    sc->err.clear();
    const size_t M = sc->polar.size();
    if (k < 1 || k > 8) return scfail(sc, "k must be 1..8, not " + std::to_string(k));
    if (first > M || count > M - first) return scfail(sc, "first + count = " + std::to_string(first) + " + " + std::to_string(count) + " exceeds the " + std::to_string(M) + " stored contexts");
    if (count == 0) return 0;
    if (!idx) return scfail(sc, "idx is NULL");
    if (!dist) return scfail(sc, "dist is NULL");
    if (!shift) return scfail(sc, "shift is NULL");
    if (sc->prm.num_exclude_recent < 0) return scfail(sc, "num_exclude_recent is negative");
    if (M > 0x7fffff00ull) return scfail(sc, "too many contexts");
    S_TRY(hipSetDevice(sc->device));
    if (sc_keys_upto(sc, first + count)) return 1;
    const int excl = sc->prm.num_exclude_recent;
    const int radius = std::min(kSectors, std::max(0, (int)round(0.5 * (double)(float)sc->prm.search_ratio * kSectors)));      // as pcr_sc_distance
    const size_t per_row = (size_t)k * (sizeof(double) + sizeof(long long) + sizeof(int));
    if (sc_room(sc, &sc->d_rank, &sc->rank_cap, count * per_row)) return 1;
    double* o_d = static_cast<double*>(sc->d_rank);
    long long* o_i = reinterpret_cast<long long*>(o_d + count * k);
    int* o_s = reinterpret_cast<int*>(o_i + count * k);
    // candidate tiles of a query: ceil((q - excl) / kTileC).  The queries go in chunks whose per-tile lists fit kPartBytes; a query's
    // row depends on no other query, so the chunking does not show in the result.
    auto tiles_of = [&](size_t q) { return q > (size_t)excl ? (q - excl + kTileC - 1) / kTileC : 0; };
    constexpr size_t kPartBytes = 64u << 20, kEntry = sizeof(double) + 2 * sizeof(int);
    const size_t fit = kPartBytes / (std::max<size_t>(1, tiles_of(first + count - 1)) * k * kEntry);
    const size_t rows = std::min<size_t>(std::max<size_t>(kTileQ, fit / kTileQ * kTileQ), (size_t)1 << 20);
    for (size_t at = 0; at < count; at += rows) {
        const size_t n = std::min(rows, count - at), nct = tiles_of(first + at + n - 1);
        if (nct) {
            if (sc_room(sc, &sc->d_part, &sc->part_cap, n * nct * k * kEntry)) return 1;
            double* p_d = static_cast<double*>(sc->d_part);
            int* p_i = reinterpret_cast<int*>(p_d + n * nct * k);
            int* p_s = p_i + n * nct * k;
            const size_t blocks = (n + kTileQ - 1) / kTileQ * nct;
            if (blocks > 0x7fffffffull) return scfail(sc, "too many tiles in one launch");
            hipLaunchKernelGGL(sc_rank_stored_kernel, dim3((unsigned int)blocks), dim3(64 * kStoredWaves), 0, 0, sc->d_db, sc->d_keys, (unsigned int)(first + at),
                               (unsigned int)n, (unsigned int)nct, excl, radius, k, p_d, p_i, p_s);
            S_TRY(hipGetLastError());
        }
        const double* p_d = static_cast<const double*>(sc->d_part);
        const int* p_i = reinterpret_cast<const int*>(p_d + n * nct * k);
        hipLaunchKernelGGL(sc_rank_merge_kernel, dim3((unsigned int)((n + 3) / 4)), dim3(256), 0, 0, p_d, p_i, p_i + n * nct * k, (unsigned int)(first + at),
                           (unsigned int)n, (unsigned int)nct, excl, k, o_i + at * k, o_d + at * k, o_s + at * k);
        S_TRY(hipGetLastError());
    }
    // into scratch first: a failed copy must leave the caller's arrays as they were
    std::vector<char> host(count * per_row);
    S_TRY(hipMemcpy(host.data(), sc->d_rank, host.size(), hipMemcpyDeviceToHost));
    const char* h = host.data();
    std::copy(reinterpret_cast<const double*>(h), reinterpret_cast<const double*>(h) + count * k, dist);
    h += count * k * sizeof(double);
    std::copy(reinterpret_cast<const long long*>(h), reinterpret_cast<const long long*>(h) + count * k, idx);
    h += count * k * sizeof(long long);
    std::copy(reinterpret_cast<const int*>(h), reinterpret_cast<const int*>(h) + count * k, shift);
    return 0;
}

/* trans::deg2rad<float> of shift sectors of 6 degrees: the yaw of a match (:276) */
float pcr_sc_shift_yaw(int32_t shift) { return (float)((double)((360.0f / (float)kSectors) * (float)shift) * 3.14159265358979323846 / 180.0); }

/* query (:231-279): *match = -1 when there is no loop candidate; yaw = deg2rad(6 deg * shift) as a float */
int pcr_sc_query(pcr_sc* sc, long long id, long long* match, float* yaw_rad, double* min_dist_out) {
    if (!sc || !match) return 1;
    sc->err.clear();
    *match = -1;
    if (yaw_rad) *yaw_rad = 0.f;
    if (min_dist_out) *min_dist_out = std::numeric_limits<double>::max();
    if (id < 0 || (size_t)id >= sc->polar.size()) return scfail(sc, "no such context");
    const long long excl = sc->prm.num_exclude_recent, ncand = sc->prm.num_candidates;
    if (id <= excl + ncand) return 0;
    // the candidate set is a snapshot, refreshed only every build_tree_gap contexts (:240-248)
    if (sc->tree_size == 0 || (size_t)id - sc->tree_size > (size_t)(excl + sc->prm.build_tree_gap)) sc->tree_size = (size_t)(id - excl);
    // exact k nearest ring keys (squared L2, ties on the lower index)
    std::vector<std::pair<double, size_t>> cand;
    for (size_t i = 0; i < sc->tree_size; ++i) {
        double s = 0;
        for (int r = 0; r < kRings; ++r) { const double d = sc->ring[(size_t)id][r] - sc->ring[i][r]; s += d * d; }
        cand.emplace_back(s, i);
    }
    const size_t k = std::min<size_t>((size_t)ncand, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + k, cand.end());
    double min_dist = std::numeric_limits<double>::max();
    int nn_align = 0;
    size_t nn_idx = 0;
    for (size_t c = 0; c < k; ++c) {
        double d; int sh;
        pcr_sc_distance(sc, (size_t)id, cand[c].second, &d, &sh);
        if (d < min_dist) { min_dist = d; nn_align = sh; nn_idx = cand[c].second; }
    }
    if (min_dist_out) *min_dist_out = min_dist;
    if (min_dist > (double)(float)sc->prm.dist_thres) return 0;
    *match = (long long)nn_idx;
    if (yaw_rad) *yaw_rad = pcr_sc_shift_yaw(nn_align);
    return 0;
}

}  // extern "C"
