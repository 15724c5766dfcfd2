// knn_query.hip -- exact k-nearest-neighbour and radius queries on the uniform-grid index of a kept target (pcr_knn, pcr_radius_search:
// capi.hip), the two operations of the reference's nanoflann::PointCloudKdtree (pcl_adaptor.hpp:47-78).
//
// Semantics: nanoflann's metric_L2_Simple with a double distance type on float coordinates.  Both coordinates are widened to f64, the
// differences are taken in f64 and d2 = dx*dx + dy*dy + dz*dz is added in that order (no contraction: -ffp-contract=off), so d2 is the
// reference's bit for bit.  Selection and order are decided on (d2, original index) alone -- there is no float screening key anywhere.
//
// What makes the searches exact on every lattice the library builds (LOAM's power-of-two cells, VGICP's lattice shifted by half a cell,
// NDT's pcl::VoxelGrid lattice whose cell index is computed in FLOAT): a point that the build put into cell i of an axis has its
// coordinate x within
//     (o + i) cell - slop  <=  x  <=  (o + i + 1) cell + slop,      o = org + shift,      slop = (|face| + |query| + cell) 2^-20.
// The f64 lattices round x / cell to 2^-53, the float one rounds x * (1 / leaf) twice to 2^-24 each: at most |x| 2^-22 metres.  The
// slop is four times that and also covers the rounding of the f64 products below.  Every bound in this file is a distance to a face
// of the block of cells ACTUALLY scanned, less the slop: it never assumes that the query lies in the centre cell (a query outside
// the grid has its centre cell clamped into it).
//
// k-NN: a lane per query for every k, instantiated for K = 1, 8, 16, 32 (the caller's k is rounded up).  The list is K (d2, index)
// pairs in registers, 3 K VGPRs; the kernels run at one or two waves per SIMD (DESIGN.md 4.10 has the resource table).
// Radius: a wave per query.  A count pass, an exclusive scan of the counts on the device (one block), a fill pass that writes each
// query's segment in storage order, and a rank sort of every segment by (d2, index) that takes any length (tiles of 1024 keys in LDS).
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "nb_list.h"
#include "sparse_walk.h"

namespace pcr {

namespace {

using sw::slab_gap;      // (the bounds of this file, shared with the sparse index's walk)
using sw::slop_of;

struct Lattice {
    int d0, d1, d2;
    double cell, shift, org[3], o[3];      // cell i of axis d spans [(o[d] + i) cell, (o[d] + i + 1) cell), up to the slop
};

__device__ __forceinline__ Lattice lattice_of(const GridHeader& h) {
    Lattice l;
    l.d0 = h.dims[0]; l.d1 = h.dims[1]; l.d2 = h.dims[2];
    l.cell = h.cell; l.shift = h.shift;
#pragma unroll
    for (int d = 0; d < 3; ++d) { l.org[d] = h.org[d]; l.o[d] = h.org[d] + h.shift; }
    return l;
}

// ---------------------------------------------------------------------------------------------------------------------------
// k nearest neighbours
// ---------------------------------------------------------------------------------------------------------------------------
// Rings 1, 2, ... around the (clamped) centre cell until the K-th distance is proven final.  Ring r adds the shell of the block
// [c - r, c + r]; ring 1 is the whole 3 x 3 x 3 block.  Every point is visited once.
template <int K>
__device__ __forceinline__ void nb_search(const Lattice& g, const float4* __restrict__ pts, const uint32_t* __restrict__ cell_start,
                                          double qx, double qy, double qz, NbList<K>& L) {
    const int d0 = g.d0, d1 = g.d1, d2 = g.d2;
    const double fx = floor(qx / g.cell - g.shift) - g.org[0], fy = floor(qy / g.cell - g.shift) - g.org[1], fz = floor(qz / g.cell - g.shift) - g.org[2];
    const int cx = (int)fmin(fmax(fx, 0.0), (double)(d0 - 1)), cy = (int)fmin(fmax(fy, 0.0), (double)(d1 - 1)), cz = (int)fmin(fmax(fz, 0.0), (double)(d2 - 1));
    const int rmax = max(max(max(cx, d0 - 1 - cx), max(cy, d1 - 1 - cy)), max(cz, d2 - 1 - cz));
    for (int r = 1; r <= max(rmax, 1); ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, d2 - 1), y0 = max(cy - r, 0), y1 = min(cy + r, d1 - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, d0 - 1);
        for (int z = z0; z <= z1; ++z) {
            const double gz = slab_gap(g.o[2], z, g.cell, qz);
            if (gz * gz > L.d[K - 1]) continue;
            // rows y0..y1 of one z layer are contiguous in key order: one subtraction tells whether the whole band is empty
            if (cell_start[((uint32_t)z * (uint32_t)d1 + (uint32_t)y0) * (uint32_t)d0] ==
                cell_start[((uint32_t)z * (uint32_t)d1 + (uint32_t)y1 + 1u) * (uint32_t)d0]) continue;
            for (int y = y0; y <= y1; ++y) {
                const double gy = slab_gap(g.o[1], y, g.cell, qy);
                if (gy * gy + gz * gz > L.d[K - 1]) continue;      // the whole row is farther than the K-th distance as it stands
                const uint32_t row = ((uint32_t)z * (uint32_t)d1 + (uint32_t)y) * (uint32_t)d0;
                const bool shell_row = r == 1 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                if (shell_row) {
                    nb_scan_run<K>(pts, cell_start[row + x0], cell_start[row + x1 + 1], qx, qy, qz, L);
                } else {
                    if (cx - r >= 0) nb_scan_run<K>(pts, cell_start[row + cx - r], cell_start[row + cx - r + 1], qx, qy, qz, L);
                    if (cx + r <= d0 - 1) nb_scan_run<K>(pts, cell_start[row + cx + r], cell_start[row + cx + r + 1], qx, qy, qz, L);
                }
            }
        }
        // Every point not yet visited lies beyond a face of the block [c - r, c + r] that is not on the grid's boundary, and the query is
        // on the near side of each such face (or in its plane's slop): its distance is at least the least of the face distances below.
        double bound = INFINITY;
        if (cx - r > 0) { const double f = (g.o[0] + (double)(cx - r)) * g.cell; bound = fmin(bound, qx - f - slop_of(f, qx, g.cell)); }
        if (cx + r < d0 - 1) { const double f = (g.o[0] + (double)(cx + r + 1)) * g.cell; bound = fmin(bound, f - qx - slop_of(f, qx, g.cell)); }
        if (cy - r > 0) { const double f = (g.o[1] + (double)(cy - r)) * g.cell; bound = fmin(bound, qy - f - slop_of(f, qy, g.cell)); }
        if (cy + r < d1 - 1) { const double f = (g.o[1] + (double)(cy + r + 1)) * g.cell; bound = fmin(bound, f - qy - slop_of(f, qy, g.cell)); }
        if (cz - r > 0) { const double f = (g.o[2] + (double)(cz - r)) * g.cell; bound = fmin(bound, qz - f - slop_of(f, qz, g.cell)); }
        if (cz + r < d2 - 1) { const double f = (g.o[2] + (double)(cz + r + 1)) * g.cell; bound = fmin(bound, f - qz - slop_of(f, qz, g.cell)); }
        if (bound == INFINITY) return;      // the block covers the whole grid
        // strictly nearer than anything unvisited: a tie with an unvisited point of lower index cannot occur
        if (bound > 0.0 && L.d[K - 1] < bound * bound * (1.0 - 0x1p-40)) return;
    }
}

template <int K, int BLOCK>
__global__ __launch_bounds__(BLOCK) void knn_query_kernel(GridView gv, const float* __restrict__ q, uint32_t n_q, uint32_t stride, int k,
                                                          int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_q) return;
    const GridHeader& h = *gv.hdr;
    NbList<K> L;
#pragma unroll
    for (int j = 0; j < K; ++j) { L.d[j] = INFINITY; L.i[j] = 0xffffffffu; }
    const float* p = q + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    if (!h.empty && isfinite(x) && isfinite(y) && isfinite(z)) nb_search<K>(lattice_of(h), gv.pts, gv.cell_start, (double)x, (double)y, (double)z, L);
    int64_t* oi = out_idx + (size_t)i * (size_t)k;
    double* od = out_d2 + (size_t)i * (size_t)k;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) { oi[j] = L.i[j] == 0xffffffffu ? (int64_t)-1 : (int64_t)L.i[j]; od[j] = L.d[j]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// radius search
// ---------------------------------------------------------------------------------------------------------------------------
// The cells of one axis that can hold a point within `radius` of q: false when there is none
__device__ __forceinline__ bool axis_range(double o_org, double shift, int dim, double cell, double q, double radius, int* lo, int* hi) {
    const double a = q - radius, b = q + radius;
    const double fl = floor((a - slop_of(a, q, cell)) / cell - shift) - o_org, fh = floor((b + slop_of(b, q, cell)) / cell - shift) - o_org;
    if (!(fh >= 0.0) || !(fl <= (double)(dim - 1))) return false;
    *lo = (int)fmax(fl, 0.0);
    *hi = (int)fmin(fh, (double)(dim - 1));
    return true;
}

// A wave per query.  FILL = false: counts[q] = number of points with d2 < r2.  FILL = true: they are written to the query's segment
// in the order the index stores them (rows by z, y; points by position) -- the same order in every call.
template <bool FILL>
__global__ __launch_bounds__(256) void radius_query_kernel(GridView gv, const float* __restrict__ q, uint32_t n_q, uint32_t stride, double radius, double r2,
                                                           uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets,
                                                           int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n_q) return;
    const GridHeader& h = *gv.hdr;
    const float* p = q + (size_t)i * stride;
    const float xf = p[0], yf = p[1], zf = p[2];
    uint32_t total = 0;
    int x0, x1, y0, y1, z0, z1;
    const double qx = (double)xf, qy = (double)yf, qz = (double)zf;
    if (!h.empty && isfinite(xf) && isfinite(yf) && isfinite(zf) &&
        axis_range(h.org[0], h.shift, h.dims[0], h.cell, qx, radius, &x0, &x1) && axis_range(h.org[1], h.shift, h.dims[1], h.cell, qy, radius, &y0, &y1) &&
        axis_range(h.org[2], h.shift, h.dims[2], h.cell, qz, radius, &z0, &z1)) {
        const unsigned long long base = FILL ? offsets[i] : 0ull;
        const uint32_t d0 = (uint32_t)h.dims[0], d1 = (uint32_t)h.dims[1];
        const double o1 = h.org[1] + h.shift, o2 = h.org[2] + h.shift;
        for (int z = z0; z <= z1; ++z) {
            const double gz = slab_gap(o2, z, h.cell, qz);
            if (gz * gz >= r2 * (1.0 + 0x1p-40)) continue;
            for (int y = y0; y <= y1; ++y) {
                const double gy = slab_gap(o1, y, h.cell, qy);
                if (gy * gy + gz * gz >= r2 * (1.0 + 0x1p-40)) continue;
                const uint32_t row = ((uint32_t)z * d1 + (uint32_t)y) * d0;
                const uint32_t s = gv.cell_start[row + (uint32_t)x0], e = gv.cell_start[row + (uint32_t)x1 + 1u];
                for (uint32_t j0 = s; j0 < e; j0 += 64) {
                    const uint32_t j = j0 + lane;
                    bool in = false;
                    double d = 0.0;
                    uint32_t idx = 0;
                    if (j < e) {
                        const float4 t = gv.pts[j];
                        const double dx = qx - (double)t.x, dy = qy - (double)t.y, dz = qz - (double)t.z;
                        d = dx * dx;
                        d += dy * dy;
                        d += dz * dz;
                        idx = __float_as_uint(t.w);
                        in = d < r2;      // strict, as RadiusResultSet::addPoint
                    }
                    const unsigned long long m = __ballot(in);
                    if (FILL && in) {
                        const unsigned long long at = base + total + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                        out_idx[at] = (int64_t)idx;
                        out_d2[at] = d;
                    }
                    total += (uint32_t)__popcll(m);
                }
            }
        }
    }
    if (!FILL && lane == 0) counts[i] = total;
}

// offsets[i] = counts[0] + ... + counts[i - 1], i = 0 .. n: one block walks the counts in chunks of 1024 with a running carry
__global__ __launch_bounds__(1024) void radius_scan_kernel(const uint32_t* __restrict__ counts, uint32_t n, unsigned long long* __restrict__ offsets) {
    __shared__ unsigned long long sh[1024];
    unsigned long long carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 1024) {
        const uint32_t i = c0 + threadIdx.x;
        const unsigned long long mine = i < n ? (unsigned long long)counts[i] : 0ull;
        unsigned long long v = mine;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int s = 1; s < 1024; s <<= 1) {
            const unsigned long long add = threadIdx.x >= (uint32_t)s ? sh[threadIdx.x - s] : 0ull;
            __syncthreads();
            v += add;
            sh[threadIdx.x] = v;
            __syncthreads();
        }
        if (i < n) offsets[i] = carry + v - mine;
        carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

// A block per query: every entry's rank among its segment's (d2, index) keys -- all distinct, an index occurs once -- is its place in
// the output.  Squared distances are >= 0, so their bit patterns order as they do.  Any length: the keys pass through LDS in tiles.
static constexpr int kSortTile = 1024;
__global__ __launch_bounds__(256) void radius_sort_kernel(const unsigned long long* __restrict__ offsets, const int64_t* __restrict__ in_idx,
                                                          const double* __restrict__ in_d2, int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    __shared__ unsigned long long sk[kSortTile];
    __shared__ uint32_t si[kSortTile];
    const unsigned long long a = offsets[blockIdx.x], b = offsets[blockIdx.x + 1];
    const unsigned long long len = b - a;
    if (len == 0) return;
    if (len == 1) { if (threadIdx.x == 0) { out_idx[a] = in_idx[a]; out_d2[a] = in_d2[a]; } return; }
    for (unsigned long long e0 = 0; e0 < len; e0 += 256) {
        const unsigned long long e = e0 + threadIdx.x;
        const bool have = e < len;
        const double md = have ? in_d2[a + e] : 0.0;
        const unsigned long long mk = (unsigned long long)__double_as_longlong(md);
        const uint32_t mi = have ? (uint32_t)in_idx[a + e] : 0u;
        unsigned long long rank = 0;
        for (unsigned long long t0 = 0; t0 < len; t0 += kSortTile) {
            const uint32_t tn = (uint32_t)(len - t0 < (unsigned long long)kSortTile ? len - t0 : (unsigned long long)kSortTile);
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < tn; j += 256) {
                sk[j] = (unsigned long long)__double_as_longlong(in_d2[a + t0 + j]);
                si[j] = (uint32_t)in_idx[a + t0 + j];
            }
            __syncthreads();
            if (have) {
                uint32_t less = 0;
                for (uint32_t j = 0; j < tn; ++j) less += (sk[j] < mk || (sk[j] == mk && si[j] < mi)) ? 1u : 0u;
                rank += less;
            }
        }
        if (have) { out_idx[a + rank] = (int64_t)mi; out_d2[a + rank] = md; }
    }
}

}  // namespace

hipError_t knn_query_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, int k, int64_t* d_idx, double* d_d2, hipStream_t s) {
    if (n_q == 0) return hipSuccess;
    if (k < 1 || k > PCR_KNN_MAX_K || n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const GridView gv = grid.view();
    const uint32_t n = (uint32_t)n_q, st = (uint32_t)stride_floats;
    // small lists: 256 queries per block; the long ones: a wave per block, so that a far query holds 63 others and not 255
    if (k == 1) hipLaunchKernelGGL((knn_query_kernel<1, 256>), dim3((n + 255) / 256), dim3(256), 0, s, gv, d_q, n, st, k, d_idx, d_d2);
    else if (k <= 8) hipLaunchKernelGGL((knn_query_kernel<8, 256>), dim3((n + 255) / 256), dim3(256), 0, s, gv, d_q, n, st, k, d_idx, d_d2);
    else if (k <= 16) hipLaunchKernelGGL((knn_query_kernel<16, 64>), dim3((n + 63) / 64), dim3(64), 0, s, gv, d_q, n, st, k, d_idx, d_d2);
    else hipLaunchKernelGGL((knn_query_kernel<32, 64>), dim3((n + 63) / 64), dim3(64), 0, s, gv, d_q, n, st, k, d_idx, d_d2);
    return hipGetLastError();
}

hipError_t radius_scan_launch(const uint32_t* d_counts, size_t n_q, unsigned long long* d_offsets, hipStream_t s) {
    if (n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(radius_scan_kernel, dim3(1), dim3(1024), 0, s, d_counts, (uint32_t)n_q, d_offsets);
    return hipGetLastError();
}

hipError_t radius_count_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, double radius, uint32_t* d_counts,
                               unsigned long long* d_offsets, hipStream_t s) {
    if (n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_q;
    if (n)
        hipLaunchKernelGGL((radius_query_kernel<false>), dim3((n + 3) / 4), dim3(256), 0, s, grid.view(), d_q, n, (uint32_t)stride_floats, radius, radius * radius,
                           d_counts, (const unsigned long long*)nullptr, (int64_t*)nullptr, (double*)nullptr);
    return radius_scan_launch(d_counts, n_q, d_offsets, s);
}

hipError_t radius_fill_launch(const GridIndex& grid, const float* d_q, size_t n_q, size_t stride_floats, double radius, const unsigned long long* d_offsets,
                              int64_t* d_idx, double* d_d2, hipStream_t s) {
    if (n_q == 0) return hipSuccess;
    if (n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_q;
    hipLaunchKernelGGL((radius_query_kernel<true>), dim3((n + 3) / 4), dim3(256), 0, s, grid.view(), d_q, n, (uint32_t)stride_floats, radius, radius * radius,
                       (uint32_t*)nullptr, d_offsets, d_idx, d_d2);
    return hipGetLastError();
}

hipError_t radius_sort_launch(size_t n_q, const unsigned long long* d_offsets, const int64_t* d_in_idx, const double* d_in_d2, int64_t* d_out_idx,
                              double* d_out_d2, hipStream_t s) {
    if (n_q == 0) return hipSuccess;
    if (n_q > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(radius_sort_kernel, dim3((uint32_t)n_q), dim3(256), 0, s, d_offsets, d_in_idx, d_in_d2, d_out_idx, d_out_d2);
    return hipGetLastError();
}

}  // namespace pcr
