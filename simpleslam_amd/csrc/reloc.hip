// reloc.hip -- the gated fitness score of many poses of one source in one pass (pcr_fitness_batch), the coarse stage of relocalisation
// (pcr_relocalize: capi.hip).
//
// Per pose the answer is pcr_fitness_gated's (vgicp.hip: fitness_kernel): the source transformed in float in PCL's order, each point's
// float 1-NN squared distance from the same ring search (ring_search.h, one level), counted when it is <= the largest float <= max_sq,
// points with a coordinate that is not finite left out, and against a cut index the same test for points whose nearest target point may
// lie beyond a cut face.  The sums are taken in the order fitness_kernel + sum_partials_kernel take them for a source of up to 512 x 256
// points, so a pose's result is bit for bit the single-pose call's there.
//
// Shape: a block is 256 source points (a "chunk" of the subset) times a tile of kTile hypotheses -- consecutive in the lattice's order,
// i.e. the same yaw and neighbouring x: their queries land in nearby cells.  Each thread loads its point once and runs the tile's
// searches one after the other; the tile's per-point results wait in LDS and one barrier later each wave folds two hypotheses.  Partial
// sums go to [hypothesis][chunk]; a second kernel folds each hypothesis in chunk order.  No atomics: the result is repeatable bit for bit.
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "ring_search.h"

namespace pcr {

static constexpr int kTile = 8;      // hypotheses per block (two per wave in the fold)

__global__ __launch_bounds__(256) void reloc_score_kernel(GridView g, const float* __restrict__ src, uint64_t n_src, uint32_t stride, uint64_t m,
                                                          const float* __restrict__ poses, uint32_t n_poses, uint32_t chunks, uint32_t tiles,
                                                          float max_range, RelocPart* __restrict__ part) {
    __shared__ float shd[kTile][256];
    __shared__ uint8_t shf[kTile][256];
    const GridHeader& gh = *g.hdr;
    const int cut = gh.clamped && !gh.empty ? gh.cut_mask : 0;
    double cut_lo[3], cut_hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        cut_lo[d] = (cut >> d) & 1 ? (gh.org[d] + kPad + gh.shift) * gh.cell : -1e300;
        cut_hi[d] = (cut >> (3 + d)) & 1 ? (gh.org[d] + gh.dims[d] - kPad + gh.shift) * gh.cell : 1e300;
    }
    // blocks b and b + 8 share an XCD (round-robin dispatch; for speed only): XCD x takes the x-th eighth of the work in order, so the tiles of
    // one chunk -- the same source points, neighbouring poses -- meet in one L2.  One work item per block (the launcher sizes the grid).
    const uint32_t work = chunks * tiles, per = (work + 7) / 8;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = (blockIdx.x % 8) * per + blockIdx.x / 8;
    if (w >= work) return;      // (the whole block: before any barrier)
    {
        const uint32_t c = (uint32_t)(w / tiles), t0 = (uint32_t)(w % tiles) * kTile;
        const uint64_t j = (uint64_t)c * 256 + threadIdx.x;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        const bool have = j < m;
        if (have) {
            const uint64_t i = m == n_src ? j : (j * n_src) / m;      // the subset i_j = floor(j n / m)
            const float* p = src + i * stride;
            p0 = p[0]; p1 = p[1]; p2 = p[2];
        }
#pragma unroll 1
        for (int k = 0; k < kTile; ++k) {
            float dc = 0.f;
            uint8_t f = 0;
            if (have && t0 + k < n_poses) {
                const float* T = poses + (size_t)(t0 + k) * 16;
                const float qx = T[0] * p0 + T[4] * p1 + T[8] * p2 + T[12];
                const float qy = T[1] * p0 + T[5] * p1 + T[9] * p2 + T[13];
                const float qz = T[2] * p0 + T[6] * p1 + T[10] * p2 + T[14];
                // a point with a coordinate that is not finite is at no finite distance from anything: not counted, nothing to prove
                if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
                    const double qd[3] = {(double)qx, (double)qy, (double)qz};
                    double margin = 1e300;
                    if (cut) {
#pragma unroll
                        for (int d = 0; d < 3; ++d) margin = fmin(margin, fmin(qd[d] - cut_lo[d], cut_hi[d] - qd[d]));
                    }
                    KeyList<1> L;
                    ring_knn<1>(one_level(g), qx, qy, qz, max_range, L);
                    float d = 3.0e38f;
                    if (L.k[0] != ~0ull) {
                        d = __uint_as_float((uint32_t)(L.k[0] >> 32));
                        if (d <= max_range) { dc = d; f |= 1; }
                    }
                    if (cut && margin < 1e29 && !(sqrt((double)d) * (1.0 + 1e-6) < margin) && !(sqrt((double)max_range) * (1.0 + 1e-6) < margin)) f |= 2;
                }
            }
            shd[k][threadIdx.x] = dc;
            shf[k][threadIdx.x] = f;
        }
        __syncthreads();
        // fitness_kernel's block sum, term for term: s = 128 and 64 through LDS, then 32 .. 1 (lane t adds lane t + s)
        for (int k = wave; k < kTile; k += 4) {
            const double a = (double)shd[k][lane] + (double)shd[k][lane + 128], b = (double)shd[k][lane + 64] + (double)shd[k][lane + 192];
            double v = a + b;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
            uint32_t cnt = 0, viol = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint8_t fq = shf[k][lane + 64 * q];
                cnt += (uint32_t)__popcll(__ballot(fq & 1));
                viol += (uint32_t)__popcll(__ballot(fq & 2));
            }
            if (lane == 0 && t0 + k < n_poses) {
                RelocPart r;
                r.sum = v; r.cnt = cnt; r.viol = viol;
                part[(size_t)(t0 + k) * chunks + c] = r;
            }
        }
    }
}

// One wave per hypothesis.  sum_partials_kernel's order: lane s < 8 sums chunks s, s + 8, s + 16, ... in turn, lane 0 then adds the
// eight in lane order.
__global__ __launch_bounds__(256) void reloc_reduce_kernel(const RelocPart* __restrict__ part, uint32_t n_poses, uint32_t chunks, RelocSum* __restrict__ out) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= n_poses) return;
    const RelocPart* row = part + (size_t)h * chunks;
    double acc = 0.0;
    unsigned long long cnt = 0, viol = 0;
    if (lane < 8) {
        uint32_t c = lane;
        for (; c + 24 < chunks; c += 32) {      // four loads in flight, added in order
            RelocPart r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = row[c + 8 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u) { acc += r[u].sum; cnt += r[u].cnt; viol += r[u].viol; }
        }
        for (; c < chunks; c += 8) { const RelocPart r = row[c]; acc += r.sum; cnt += r.cnt; viol += r.viol; }
    }
    double tot = __shfl(acc, 0);
#pragma unroll
    for (int s = 1; s < 8; ++s) tot += __shfl(acc, s);
#pragma unroll
    for (int s = 4; s >= 1; s >>= 1) { cnt += __shfl_down(cnt, s); viol += __shfl_down(viol, s); }
    if (lane == 0) { RelocSum o; o.sum = tot; o.cnt = cnt; o.viol = viol; o.pad_ = 0; out[h] = o; }
}

hipError_t fitness_batch_launch(const GridIndex& grid, const float* d_src, size_t n_src, size_t stride_floats, size_t m, const float* d_poses,
                                size_t n_poses, double max_sq, RelocPart* d_part, RelocSum* d_out, hipStream_t s) {
    if (n_poses == 0) return hipSuccess;
    // the gate as fitness_launch sets it: the largest float not above max_sq
    float mr = max_sq >= (double)FLT_MAX ? FLT_MAX : (float)max_sq;
    if ((double)mr > max_sq) mr = nextafterf(mr, -FLT_MAX);
    const uint32_t chunks = (uint32_t)((m + 255) / 256), tiles = (uint32_t)((n_poses + kTile - 1) / kTile);
    const uint64_t work = (uint64_t)chunks * tiles;
    if (work > (1u << 21)) return hipErrorInvalidValue;      // (capi.hip keeps chunks x poses <= 2^21: one block per work item)
    const uint64_t nb = 8 * ((work + 7) / 8);
    if (chunks > 0)
        hipLaunchKernelGGL(reloc_score_kernel, dim3((uint32_t)nb), dim3(256), 0, s, grid.view(), d_src, (uint64_t)n_src, (uint32_t)stride_floats, (uint64_t)m,
                           d_poses, (uint32_t)n_poses, chunks, tiles, mr, d_part);
    return fitness_batch_reduce_launch(d_part, n_poses, chunks, d_out, s);
}

// (the second launch of every batched score: here and sparse_fitness.hip)
hipError_t fitness_batch_reduce_launch(const RelocPart* d_part, size_t n_poses, uint32_t chunks, RelocSum* d_out, hipStream_t s) {
    hipLaunchKernelGGL(reloc_reduce_kernel, dim3((uint32_t)((n_poses + 3) / 4)), dim3(256), 0, s, d_part, (uint32_t)n_poses, chunks, d_out);
    return hipGetLastError();
}

}  // namespace pcr
