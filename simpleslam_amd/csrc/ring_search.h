// ring_search.h -- exact k-nearest-neighbour search on the uniform grid index (GridView / GridLevels), shared by the kernels
// that query a target: the VGICP covariances and the fitness score (vgicp.hip), the batched fitness score (reloc.hip).
#pragma once
#include <math.h>

#include "pcr_internal.h"

namespace pcr {

// ------------------------------------------------------------------------------
// exact K nearest neighbours by ring search; float squared distances (x,y,z order, no FMA:
// FLANN L2_Simple<float>), ties on the lower original index.  key = dist_bits << 32 | index.
// ------------------------------------------------------------------------------
template <int K>
struct KeyList {
    unsigned long long k[K];
};

template <int K, bool DEDUPE>
__device__ __forceinline__ void keylist_insert(KeyList<K>& L, unsigned long long key) {
    bool c[K];
    bool dup = false;
#pragma unroll
    for (int i = 0; i < K; ++i) { c[i] = key < L.k[i]; if (DEDUPE) dup |= key == L.k[i]; }
    if (DEDUPE && dup) return;      // a coarser level meets the points of the finer ones again
#pragma unroll
    for (int i = K - 1; i >= 1; --i) L.k[i] = c[i - 1] ? L.k[i - 1] : (c[i] ? key : L.k[i]);
    L.k[0] = c[0] ? key : L.k[0];
}

template <int K, bool DEDUPE>
__device__ __forceinline__ void ring_scan_run(const float4* __restrict__ pts, uint32_t s, uint32_t e, float qx, float qy, float qz,
                                              KeyList<K>& L) {
    // four candidates per step, their loads issued together: with one load per iteration the branchy insertion kept the
    // compiler from overlapping them, and every candidate cost a full memory round trip
    for (uint32_t j = s; j < e; j += 4) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[j + u < e ? j + u : j];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
            float d = dx * dx;
            d += dy * dy;
            d += dz * dz;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(p[u].w);
            if (j + u < e && key < L.k[K - 1]) keylist_insert<K, DEDUPE>(L, key);
        }
    }
}

// One cloud indexed at up to three cell sizes (capi.hip: cov_levels -- a scan gets two, cell and 6 cell).  A lidar scan spans four
// orders of magnitude of density; on a single grid the K-neighbourhood of a far point is dozens of rings wide and one such
// lane holds its whole wave.  Rings 1 and 2 of each level guarantee radii of one and two of its cells; only the last level
// keeps growing.
struct GridLevels {
    const GridHeader* hdr[3];
    const float4* pts[3];
    const uint32_t* cell_start[3];
    int n;
};

// Rings first..last of one level.  Returns true when the K-th distance is final (or nothing can lie beyond).
static constexpr bool kBatchRing1 = true;      // (taken only where the caller hands an LDS table over)
// rows: 9 x 256 uint2 of LDS (this block's), or nullptr (callers outside a 256-thread block layout)
template <int K, bool DEDUPE>
__device__ __forceinline__ bool ring_level(const GridHeader& h, const float4* __restrict__ pts, const uint32_t* __restrict__ cell_start,
                                           float qx, float qy, float qz, float max_sq, int last_ring, KeyList<K>& L, uint2* rows = nullptr) {
    const int d0 = h.dims[0], d1 = h.dims[1], d2 = h.dims[2];
    double fx = floor((double)qx / h.cell - h.shift) - h.org[0], fy = floor((double)qy / h.cell - h.shift) - h.org[1],
           fz = floor((double)qz / h.cell - h.shift) - h.org[2];
    // centre cell, clamped into the grid (queries of the fitness score may lie outside)
    const int cx = (int)fmin(fmax(fx, 0.0), (double)(d0 - 1)), cy = (int)fmin(fmax(fy, 0.0), (double)(d1 - 1)),
              cz = (int)fmin(fmax(fz, 0.0), (double)(d2 - 1));
    const int rmax = max(max(max(cx, d0 - 1 - cx), max(cy, d1 - 1 - cy)), max(cz, d2 - 1 - cz));
    const float cellf = (float)h.cell;
    const double o0 = h.org[0] + h.shift, o1 = h.org[1] + h.shift, o2 = h.org[2] + h.shift;   // cell i spans [(o + i) cell, (o + i + 1) cell)
    for (int r = 1; r <= max(rmax, 1); ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, d2 - 1), y0 = max(cy - r, 0), y1 = min(cy + r, d1 - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, d0 - 1);
        const float worst = __uint_as_float((uint32_t)(L.k[K - 1] >> 32));
        if (kBatchRing1 && r == 1 && rows) {
            // Ring 1 -- the nine rows of the 3 x 3 x 3 block, for most points the whole search of a level -- with ALL its row ranges
            // requested at once (18 independent loads) instead of row by row: a scan point's search is a chain of dependent round
            // trips at one wave per SIMD, and the nine pairs were nine of them.  The ranges wait in this lane's slots of the block's
            // LDS table; rows are then walked in the same order, each tested against the K-th distance as it stands.
            uint32_t ra[9], rb[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int z = cz + i / 3 - 1, y = cy + i % 3 - 1;
                const bool in = z >= 0 && z < d2 && y >= 0 && y < d1;
                const uint32_t row = in ? ((uint32_t)z * (uint32_t)d1 + (uint32_t)y) * (uint32_t)d0 : 0u;
                ra[i] = cell_start[in ? row + (uint32_t)x0 : 0u]; rb[i] = cell_start[in ? row + (uint32_t)x1 + 1u : 0u];
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) rows[i * 256 + threadIdx.x] = make_uint2(ra[i], rb[i]);
            for (int i = 0; i < 9; ++i) {
                const uint2 rg = rows[i * 256 + threadIdx.x];      // (each lane reads back what it wrote: no barrier)
                if (rg.y <= rg.x) continue;
                const int z = cz + i / 3 - 1, y = cy + i % 3 - 1;
                const float zlo = (float)((o2 + z) * h.cell), gz = fmaxf(fmaxf(zlo - qz, qz - (zlo + cellf)), 0.f) * 0.99999f;
                const float ylo = (float)((o1 + y) * h.cell), gy = fmaxf(fmaxf(ylo - qy, qy - (ylo + cellf)), 0.f) * 0.99999f;
                if (gy * gy + gz * gz > __uint_as_float((uint32_t)(L.k[K - 1] >> 32))) continue;
                ring_scan_run<K, DEDUPE>(pts, rg.x, rg.y, qx, qy, qz, L);
            }
        } else
        for (int z = z0; z <= z1; ++z) {
            // distance from the query to the slab of cells z (0 inside it); float, shaved so that it never exceeds the true gap
            const float zlo = (float)((o2 + z) * h.cell), gz = fmaxf(fmaxf(zlo - qz, qz - (zlo + cellf)), 0.f) * 0.99999f;
            if (gz * gz > worst) continue;
            // rows y0..y1 of one z layer are contiguous in key order: one subtraction tells whether the whole band
            // (all x) is empty
            if (cell_start[((uint32_t)z * (uint32_t)d1 + (uint32_t)y0) * (uint32_t)d0] ==
                cell_start[((uint32_t)z * (uint32_t)d1 + (uint32_t)y1 + 1u) * (uint32_t)d0]) continue;
            for (int y = y0; y <= y1; ++y) {
                const float ylo = (float)((o1 + y) * h.cell), gy = fmaxf(fmaxf(ylo - qy, qy - (ylo + cellf)), 0.f) * 0.99999f;
                if (gy * gy + gz * gz > worst) continue;      // the whole row is farther than the current K-th distance
                const uint32_t row = ((uint32_t)z * (uint32_t)d1 + (uint32_t)y) * (uint32_t)d0;
                const bool shell_row = r == 1 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                if (shell_row) {
                    ring_scan_run<K, DEDUPE>(pts, cell_start[row + x0], cell_start[row + x1 + 1], qx, qy, qz, L);
                } else {
                    if (cx - r >= 0) ring_scan_run<K, DEDUPE>(pts, cell_start[row + cx - r], cell_start[row + cx - r + 1], qx, qy, qz, L);
                    if (cx + r <= d0 - 1) ring_scan_run<K, DEDUPE>(pts, cell_start[row + cx + r], cell_start[row + cx + r + 1], qx, qy, qz, L);
                }
            }
        }
        // every point not yet visited lies beyond a face of the block [c-r, c+r]; faces on the
        // grid boundary have nothing behind them
        double bound = 1e300;
        if (cx - r > 0) bound = fmin(bound, (double)qx - (o0 + (double)(cx - r)) * h.cell);
        if (cx + r < d0 - 1) bound = fmin(bound, (o0 + (double)(cx + r + 1)) * h.cell - (double)qx);
        if (cy - r > 0) bound = fmin(bound, (double)qy - (o1 + (double)(cy - r)) * h.cell);
        if (cy + r < d1 - 1) bound = fmin(bound, (o1 + (double)(cy + r + 1)) * h.cell - (double)qy);
        if (cz - r > 0) bound = fmin(bound, (double)qz - (o2 + (double)(cz - r)) * h.cell);
        if (cz + r < d2 - 1) bound = fmin(bound, (o2 + (double)(cz + r + 1)) * h.cell - (double)qz);
        if (bound >= 1e299) return true;   // the block covers the whole grid
        const double b2 = bound > 0 ? bound * bound * (1.0 - 1e-5) : 0.0;   // margin: float distances
        if (b2 > (double)max_sq) return true;
        if ((double)__uint_as_float((uint32_t)(L.k[K - 1] >> 32)) < b2) return true;
        if (r >= last_ring) return false;
    }
    return true;
}

// Exact K nearest neighbours.  max_sq: neighbours farther than this are not needed (FLT_MAX for none).
// seed_sq: a radius^2 expected to hold at least K points (from the local density); the list starts with
// sentinels at that radius so that, in a crowded cell, the thousands of farther candidates are rejected by one
// compare instead of being inserted and displaced again.
template <int K>
__device__ __forceinline__ void ring_knn_pass(const GridLevels& lv, float qx, float qy, float qz, float max_sq, float seed_sq, KeyList<K>& L, uint2* rows) {
    const unsigned long long sentinel = ((unsigned long long)__float_as_uint(seed_sq) << 32) | 0xffffffffull;
#pragma unroll
    for (int i = 0; i < K; ++i) L.k[i] = sentinel;
    bool done = ring_level<K, false>(*lv.hdr[0], lv.pts[0], lv.cell_start[0], qx, qy, qz, max_sq, lv.n > 1 ? 2 : 0x7fffffff, L, rows);
    for (int l = 1; l < lv.n; ++l) {
        if (done) break;
        done = ring_level<K, true>(*lv.hdr[l], lv.pts[l], lv.cell_start[l], qx, qy, qz, max_sq, l + 1 < lv.n ? 2 : 0x7fffffff, L, rows);
    }
}

template <int K>
__device__ __forceinline__ void ring_knn(const GridLevels& lv, float qx, float qy, float qz, float max_sq, KeyList<K>& L, uint2* rows = nullptr) {
    const GridHeader& h = *lv.hdr[0];
    if (h.empty || h.overflow) {
#pragma unroll
        for (int i = 0; i < K; ++i) L.k[i] = ~0ull;
        return;
    }
    float seed = 3.0e38f;
    if (K > 1) {
        // points of the query's own cell, taken as a surface patch of area cell^2: radius holding ~2K of them
        const double fx = floor((double)qx / h.cell - h.shift) - h.org[0], fy = floor((double)qy / h.cell - h.shift) - h.org[1],
                     fz = floor((double)qz / h.cell - h.shift) - h.org[2];
        if (fx >= 0 && fx < h.dims[0] && fy >= 0 && fy < h.dims[1] && fz >= 0 && fz < h.dims[2]) {
            const uint32_t key = ((uint32_t)fz * (uint32_t)h.dims[1] + (uint32_t)fy) * (uint32_t)h.dims[0] + (uint32_t)fx;
            const uint32_t nc = lv.cell_start[0][key + 1] - lv.cell_start[0][key];
            if (nc >= 4u * (uint32_t)K) seed = (float)(h.cell * h.cell) * (2.0f * (float)K / (3.14159265f * (float)nc));
        }
    }
    ring_knn_pass<K>(lv, qx, qy, qz, max_sq, seed, L, rows);
    if (seed < 3.0e38f && (uint32_t)L.k[K - 1] == 0xffffffffu)      // the seed radius held fewer than K points: exact redo
        ring_knn_pass<K>(lv, qx, qy, qz, max_sq, 3.0e38f, L, rows);
#pragma unroll
    for (int i = 0; i < K; ++i) if ((uint32_t)L.k[i] == 0xffffffffu) L.k[i] = ~0ull;   // unfilled slots
}

__device__ __forceinline__ GridLevels one_level(const GridView& g) {
    GridLevels lv;
    lv.hdr[0] = lv.hdr[1] = lv.hdr[2] = g.hdr; lv.pts[0] = lv.pts[1] = lv.pts[2] = g.pts;
    lv.cell_start[0] = lv.cell_start[1] = lv.cell_start[2] = g.cell_start; lv.n = 1;
    return lv;
}

}  // namespace pcr
