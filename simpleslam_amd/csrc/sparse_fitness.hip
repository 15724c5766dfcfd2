// sparse_fitness.hip -- the fitness scores on the sparse target index (gfx950): pcr_fitness, pcr_fitness_gated, pcr_fitness_batch and the scores of
// relocalisation on a target whose dense index was cut (two sessions 30 km apart, a stray return at 4e6 m), or wherever the caller asks for the
// sparse index (pcr_params.query_index: query_host.hip, fitness_host.hip).
//
// Two kernels, the twins of vgicp.hip's fitness_kernel and reloc.hip's reloc_score_kernel: the same float transform, the same gate, the same
// launch shape (256 threads, the same point of the source to the same thread of the same block), the same fixed-order sums in double, the same
// outputs.  Only the search differs: sparse_walk.h's k-NN walk with K = 1 under sw::NearestF32, which finds the least FLOAT squared distance --
// the score's metric, not pcr_knn's (the rounding argument stands at the visitor).  That least distance is one value whichever index finds it, so
// with the same order of summation a score is the dense kernel's bit for bit wherever the dense kernel answers.  The index holds every finite point
// of the target: the count of points whose neighbour may have been cut off (viol) is always 0.
//
// A lane per source point, the walk a chain of dependent binary searches (log2 n steps of one 8-byte load each): latency, not bandwidth.  Nothing is
// staged in LDS -- the lanes of a wave search different rows -- and the keys of a map of a million points (8 MB) stay in L2; what hides the latency is
// occupancy, so the kernels hold no arrays and the batched one keeps its tile's results in LDS, not in registers (profiles/sparse_fitness_notes.md
// has the register, scratch and LDS figures).  No atomics: a result is repeatable bit for bit.
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"

namespace pcr {

namespace {

struct SfPose { float m[16]; };
static constexpr int kSfTile = 8;      // hypotheses per block of the batched kernel: reloc.hip's kTile (the fold below takes two per wave)

// the float squared distance from (qx, qy, qz) to the nearest stored point when that is <= max_range, else sw::NearestF32::kNone
__device__ __forceinline__ float sf_nearest(const sw::View& v, float qx, float qy, float qz, float max_range) {
    sw::NearestF32 vis;
    vis.start(v.pts, qx, qy, qz, max_range);
    sw::NoStats st;
    sw::knn_walk(v, (double)qx, (double)qy, (double)qz, 1u, vis, st);
    return vis.best;
}

// fitness_kernel's arguments less the tile, and its outputs: partials[block][32], [0] the sum, [1] the count, [2] = 0
__global__ __launch_bounds__(256) void sparse_fitness_kernel(sw::View v, const float* __restrict__ src, uint32_t n_src, uint32_t stride,
                                                             const SfPose T, float max_range, double* __restrict__ partials) {
    __shared__ double sh[256];
    __shared__ double shc[256];
    double acc = 0.0, cnt = 0.0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_src; i += gridDim.x * 256) {
        const float* p = src + (size_t)i * stride;
        const float qx = T.m[0] * p[0] + T.m[4] * p[1] + T.m[8] * p[2] + T.m[12];
        const float qy = T.m[1] * p[0] + T.m[5] * p[1] + T.m[9] * p[2] + T.m[13];
        const float qz = T.m[2] * p[0] + T.m[6] * p[1] + T.m[10] * p[2] + T.m[14];
        if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) continue;      // at no finite distance from anything
        const float d = sf_nearest(v, qx, qy, qz, max_range);
        if (d <= max_range) { acc += (double)d; cnt += 1.0; }
    }
    sh[threadIdx.x] = acc; shc[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) { sh[threadIdx.x] += sh[threadIdx.x + s]; shc[threadIdx.x] += shc[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[(size_t)blockIdx.x * 32] = sh[0]; partials[(size_t)blockIdx.x * 32 + 1] = shc[0];
        for (int k = 2; k < 32; ++k) partials[(size_t)blockIdx.x * 32 + k] = 0.0;
    }
}

// reloc_score_kernel's arguments and outputs: a block is 256 points of the subset times a tile of kSfTile poses, one work item per block, the XCD
// placement and the fold term for term as there
__global__ __launch_bounds__(256) void sparse_reloc_score_kernel(sw::View v, const float* __restrict__ src, uint64_t n_src, uint32_t stride, uint64_t m,
                                                                 const float* __restrict__ poses, uint32_t n_poses, uint32_t chunks, uint32_t tiles,
                                                                 float max_range, RelocPart* __restrict__ part) {
    __shared__ float shd[kSfTile][256];
    __shared__ uint8_t shf[kSfTile][256];
    const uint32_t work = chunks * tiles, per = (work + 7) / 8;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = (blockIdx.x % 8) * per + blockIdx.x / 8;
    if (w >= work) return;      // (the whole block: before any barrier)
    const uint32_t c = (uint32_t)(w / tiles), t0 = (uint32_t)(w % tiles) * kSfTile;
    const uint64_t j = (uint64_t)c * 256 + threadIdx.x;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    const bool have = j < m;
    if (have) {
        const uint64_t i = m == n_src ? j : (j * n_src) / m;      // the subset i_j = floor(j n / m)
        const float* p = src + i * stride;
        p0 = p[0]; p1 = p[1]; p2 = p[2];
    }
#pragma unroll 1
    for (int k = 0; k < kSfTile; ++k) {
        float dc = 0.f;
        uint8_t f = 0;
        if (have && t0 + k < n_poses) {
            const float* T = poses + (size_t)(t0 + k) * 16;
            const float qx = T[0] * p0 + T[4] * p1 + T[8] * p2 + T[12];
            const float qy = T[1] * p0 + T[5] * p1 + T[9] * p2 + T[13];
            const float qz = T[2] * p0 + T[6] * p1 + T[10] * p2 + T[14];
            if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
                const float d = sf_nearest(v, qx, qy, qz, max_range);
                if (d <= max_range) { dc = d; f = 1; }
            }
        }
        shd[k][threadIdx.x] = dc;
        shf[k][threadIdx.x] = f;
    }
    __syncthreads();
    // fitness_kernel's block sum, term for term: s = 128 and 64 through LDS, then 32 .. 1 (lane t adds lane t + s)
    for (int k = wave; k < kSfTile; k += 4) {
        const double a = (double)shd[k][lane] + (double)shd[k][lane + 128], b = (double)shd[k][lane + 64] + (double)shd[k][lane + 192];
        double s = a + b;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o);
        uint32_t cnt = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt += (uint32_t)__popcll(__ballot(shf[k][lane + 64 * q] & 1));
        if (lane == 0 && t0 + k < n_poses) {
            RelocPart r;
            r.sum = s; r.cnt = cnt; r.viol = 0;
            part[(size_t)(t0 + k) * chunks + c] = r;
        }
    }
}

// the gate as fitness_launch sets it: the largest float not above max_sq
float sf_gate(double max_sq) {
    float mr = max_sq >= (double)FLT_MAX ? FLT_MAX : (float)max_sq;
    if ((double)mr > max_sq) mr = nextafterf(mr, -FLT_MAX);
    return mr;
}

}  // namespace

hipError_t sparse_fitness_launch(const sw::View& v, const float* d_src, size_t n_src, size_t stride_floats, const double pose[16], double max_range,
                                 double* d_partials, double* d_out32, hipStream_t s, double seq) {
    SfPose T;
    for (int i = 0; i < 16; ++i) T.m[i] = (float)pose[i];
    const uint32_t nb = vgicp_blocks((uint32_t)n_src);
    hipLaunchKernelGGL(sparse_fitness_kernel, dim3(nb), dim3(256), 0, s, v, d_src, (uint32_t)n_src, (uint32_t)stride_floats, T, sf_gate(max_range), d_partials);
    return sum_partials_launch(d_partials, nb, d_out32, s, seq);
}

hipError_t sparse_fitness_batch_launch(const sw::View& v, const float* d_src, size_t n_src, size_t stride_floats, size_t m, const float* d_poses,
                                       size_t n_poses, double max_sq, RelocPart* d_part, RelocSum* d_out, hipStream_t s) {
    if (n_poses == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)((m + 255) / 256), tiles = (uint32_t)((n_poses + kSfTile - 1) / kSfTile);
    const uint64_t work = (uint64_t)chunks * tiles;
    if (work > (1u << 21)) return hipErrorInvalidValue;      // (query_host.hip keeps chunks x poses <= 2^21: one block per work item)
    const uint64_t nb = 8 * ((work + 7) / 8);
    if (chunks > 0)
        hipLaunchKernelGGL(sparse_reloc_score_kernel, dim3((uint32_t)nb), dim3(256), 0, s, v, d_src, (uint64_t)n_src, (uint32_t)stride_floats, (uint64_t)m,
                           d_poses, (uint32_t)n_poses, chunks, tiles, sf_gate(max_sq), d_part);
    return fitness_batch_reduce_launch(d_part, n_poses, chunks, d_out, s);
}

}  // namespace pcr
