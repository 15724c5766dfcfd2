// sparse_index.hip -- the sparse target index (gfx950): exact k-NN and radius queries on a target whose box no dense cell table can hold
// (pcr_knn / pcr_radius_search under pcr_params.query_index: query_host.hip).
//
// Build: the box of the finite rows (min / max of the float coordinates through an order-preserving integer code: atomics whose result does
// not depend on their order), the key layout from it and key + row per input row (sparse_walk.h: Layout, key_of; the cell floor(x / cell) in
// f64, as the dense LOAM lattice), the stable radix sort of voxel_sparse.hip (key_sort_launch), and a gather of the points into key order
// as (x, y, z, row).  Nothing is sized by the box: 24 bytes per point stay, the sort's scratch goes.  The layout and the number of stored
// points are only known on the device; the last launch writes them into page-locked memory and the host synchronises once.
// Queries: the walk of sparse_walk.h under the visitors below -- a lane per query with the list in registers for the k-NN (nb_list.h, as
// knn_query.hip), a wave per query for the radius count and fill passes.  The semantics are knn_query.hip's to the bit.
#include <math.h>

#include "pcr_internal.h"
#include "nb_list.h"

namespace pcr {

namespace {

static constexpr int kSiTile = 2048;      // rows per block of the box, key and gather passes: 8 rounds of 256

struct SiHdr {
    KeySortCtl sort;
    uint32_t mn[3], mx[3];      // ordered codes of the least / greatest finite coordinate per axis
    sw::Layout lay;
};

// float -> uint32 that orders as the floats do (finite values)
__device__ __forceinline__ uint32_t si_code(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float si_decode(uint32_t c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }
__device__ __forceinline__ bool si_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ __launch_bounds__(64) void si_init_kernel(SiHdr* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    hdr->sort.kept = 0; hdr->sort.passes = 0;
    for (int a = 0; a < 3; ++a) { hdr->mn[a] = 0xffffffffu; hdr->mx[a] = 0u; }
}

__global__ __launch_bounds__(256) void si_box_kernel(const float* __restrict__ pts, uint32_t sf, uint32_t n, SiHdr* __restrict__ hdr) {
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    const uint32_t base = blockIdx.x * kSiTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j >= n) continue;
        const float* p = pts + (size_t)j * sf;
        const float c[3] = {p[0], p[1], p[2]};
        if (!si_finite3(c[0], c[1], c[2])) continue;
        for (int a = 0; a < 3; ++a) { const uint32_t u = si_code(c[a]); mn[a] = min(mn[a], u); mx[a] = max(mx[a], u); }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], (uint32_t)__shfl_xor((int)mn[a], m, 64)); mx[a] = max(mx[a], (uint32_t)__shfl_xor((int)mx[a], m, 64)); }
    if ((threadIdx.x & 63) == 0 && mn[0] <= mx[0])
        for (int a = 0; a < 3; ++a) { atomicMin(&hdr->mn[a], mn[a]); atomicMax(&hdr->mx[a], mx[a]); }
}

__global__ __launch_bounds__(256) void si_key_kernel(const float* __restrict__ pts, uint32_t sf, uint32_t n, double cell, SiHdr* __restrict__ hdr,
                                                     unsigned long long* __restrict__ key, uint32_t* __restrict__ row) {
    __shared__ sw::Layout sh;
    __shared__ int sh_passes;
    if (threadIdx.x == 0) {
        sw::Layout l;
        int passes;
        if (hdr->mn[0] > hdr->mx[0]) {      // no finite row: the first pass still runs and counts none kept
            const double z[3] = {0.0, 0.0, 0.0};
            l = sw::layout_of(z, z);
            passes = 1;
        } else {
            double lo[3], hi[3];
            for (int a = 0; a < 3; ++a) { lo[a] = floor((double)si_decode(hdr->mn[a]) / cell); hi[a] = floor((double)si_decode(hdr->mx[a]) / cell); }
            l = sw::layout_of(lo, hi);
            const int bits = l.b[0] + l.b[1] + l.b[2];
            passes = l.refused ? 0 : (bits ? (bits + 7) / 8 : 1);
        }
        sh = l; sh_passes = passes;
        if (blockIdx.x == 0) { hdr->lay = l; hdr->sort.passes = passes; }      // (every block computes the same from the same box; the later launches read it from here)
    }
    __syncthreads();
    if (sh_passes == 0) return;
    const uint32_t base = blockIdx.x * kSiTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j >= n) continue;
        const float* p = pts + (size_t)j * sf;
        const float c[3] = {p[0], p[1], p[2]};
        const bool keep = si_finite3(c[0], c[1], c[2]);
        unsigned long long k = 0;
        if (keep) {
            unsigned long long rel[3];
            for (int a = 0; a < 3; ++a) rel[a] = (unsigned long long)((long long)floor((double)c[a] / cell) - sh.lo[a]);      // (inside the box: 0 .. ext - 1)
            k = (((rel[2] << sh.b[1]) | rel[1]) << sh.b[0]) | rel[0];
        }
        key[j] = k;
        row[j] = keep ? j : kVsDropped;
    }
}

__global__ __launch_bounds__(256) void si_gather_kernel(const SiHdr* __restrict__ hdr, const unsigned long long* __restrict__ key0,
                                                        const unsigned long long* __restrict__ key1, const uint32_t* __restrict__ row0,
                                                        const uint32_t* __restrict__ row1, const float* __restrict__ pts, uint32_t sf,
                                                        unsigned long long* __restrict__ keys_out, sw::Point* __restrict__ pts_out,
                                                        SiResult* __restrict__ result) {
    const uint32_t kept = hdr->sort.kept;
    if (blockIdx.x == 0 && threadIdx.x == 0) { SiResult r; r.kept = kept; r.pad_ = 0; r.lay = hdr->lay; *result = r; }
    const unsigned long long* key = (hdr->sort.passes & 1) ? key1 : key0;
    const uint32_t* row = (hdr->sort.passes & 1) ? row1 : row0;
    const uint32_t base = blockIdx.x * kSiTile;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t j = base + r * 256 + threadIdx.x;
        if (j >= kept) continue;
        const uint32_t rw = row[j];
        const float* p = pts + (size_t)rw * sf;
        sw::Point o;
        o.x = p[0]; o.y = p[1]; o.z = p[2]; o.row = rw;
        keys_out[j] = key[j];
        pts_out[j] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k nearest neighbours: a lane per query
// ---------------------------------------------------------------------------------------------------------------------------
template <int K>
struct KnnVisitor {
    NbList<K> L;
    const float4* pts;
    double qx, qy, qz, capv;
    __device__ __forceinline__ bool skip(double g2) const { return g2 > fmin(L.d[K - 1], capv); }
    __device__ __forceinline__ double kth() const { return L.d[K - 1]; }
    __device__ __forceinline__ void cap(double r2) { capv = r2; }
    __device__ __forceinline__ void run(uint32_t s, uint32_t e) { nb_scan_run<K>(pts, s, e, qx, qy, qz, L); }
    __device__ __forceinline__ double max_d2(uint32_t s, uint32_t e) const {
        double m = 0.0;
        for (uint32_t j = s; j < e; ++j) {
            const float4 p = pts[j];
            const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
            double d = dx * dx;
            d += dy * dy;
            d += dz * dz;
            m = fmax(m, d);
        }
        return m;
    }
};

template <int K, int BLOCK>
__global__ __launch_bounds__(BLOCK) void knn_sparse_kernel(sw::View v, const float* __restrict__ q, uint32_t n_q, uint32_t stride, int k,
                                                           int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_q) return;
    KnnVisitor<K> vis;
#pragma unroll
    for (int j = 0; j < K; ++j) { vis.L.d[j] = INFINITY; vis.L.i[j] = 0xffffffffu; }
    const float* p = q + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    vis.pts = reinterpret_cast<const float4*>(v.pts);
    vis.qx = (double)x; vis.qy = (double)y; vis.qz = (double)z; vis.capv = INFINITY;
    sw::NoStats st;
    if (isfinite(x) && isfinite(y) && isfinite(z)) sw::knn_walk(v, vis.qx, vis.qy, vis.qz, (uint32_t)K, vis, st);
    int64_t* oi = out_idx + (size_t)i * (size_t)k;
    double* od = out_d2 + (size_t)i * (size_t)k;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) { oi[j] = vis.L.i[j] == 0xffffffffu ? (int64_t)-1 : (int64_t)vis.L.i[j]; od[j] = vis.L.d[j]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// radius search: a wave per query, every lane walks the same rows
// ---------------------------------------------------------------------------------------------------------------------------
template <bool FILL>
struct RadiusVisitor {
    const float4* pts;
    double qx, qy, qz, r2;
    unsigned long long base;
    int64_t* out_idx;
    double* out_d2;
    uint32_t total, lane;
    __device__ __forceinline__ bool skip(double g2) const { return g2 >= r2 * (1.0 + 0x1p-40); }
    __device__ __forceinline__ void run(uint32_t s, uint32_t e) {
        for (uint32_t j0 = s; j0 < e; j0 += 64) {
            const uint32_t j = j0 + lane;
            bool in = false;
            double d = 0.0;
            uint32_t idx = 0;
            if (j < e) {
                const float4 t = pts[j];
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
};

// FILL = false: counts[q] = number of points with d2 < r2.  FILL = true: they are written to the query's segment in key order -- the same
// order in every call.
template <bool FILL>
__global__ __launch_bounds__(256) void radius_sparse_kernel(sw::View v, const float* __restrict__ q, uint32_t n_q, uint32_t stride, double radius, double r2,
                                                            uint32_t* __restrict__ counts, const unsigned long long* __restrict__ offsets,
                                                            int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_q) return;      // (wave-uniform)
    const float* p = q + (size_t)i * stride;
    const float xf = p[0], yf = p[1], zf = p[2];
    RadiusVisitor<FILL> vis;
    vis.pts = reinterpret_cast<const float4*>(v.pts);
    vis.qx = (double)xf; vis.qy = (double)yf; vis.qz = (double)zf; vis.r2 = r2;
    vis.base = FILL ? offsets[i] : 0ull;
    vis.out_idx = out_idx; vis.out_d2 = out_d2;
    vis.total = 0; vis.lane = threadIdx.x & 63;
    sw::NoStats st;
    if (isfinite(xf) && isfinite(yf) && isfinite(zf)) sw::radius_walk(v, vis.qx, vis.qy, vis.qz, radius, vis, st);
    if (!FILL && vis.lane == 0) counts[i] = vis.total;
}

}  // namespace

hipError_t sparse_index_build_launch(const SiBuffers& b, const float* d_src, size_t stride_floats, size_t n, unsigned long long* d_keys, sw::Point* d_pts,
                                     SiResult* result_mapped, hipStream_t s) {
    static_assert(sizeof(SiHdr) <= 256, "the header's buffer");
    if (n > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n32 = (uint32_t)n, sf = (uint32_t)stride_floats;
    const int tiles = (int)((n + kSiTile - 1) / kSiTile ? (n + kSiTile - 1) / kSiTile : 1);
    SiHdr* hdr = static_cast<SiHdr*>(b.hdr);
    hipLaunchKernelGGL(si_init_kernel, dim3(1), dim3(64), 0, s, hdr);
    hipLaunchKernelGGL(si_box_kernel, dim3(tiles), dim3(256), 0, s, d_src, sf, n32, hdr);
    hipLaunchKernelGGL(si_key_kernel, dim3(tiles), dim3(256), 0, s, d_src, sf, n32, kSparseCell, hdr, b.key[0], b.row[0]);
    key_sort_launch(&hdr->sort, n, b.key, b.row, b.hist, s);
    hipLaunchKernelGGL(si_gather_kernel, dim3(tiles), dim3(256), 0, s, hdr, b.key[0], b.key[1], b.row[0], b.row[1], d_src, sf, d_keys, d_pts, result_mapped);
    return hipGetLastError();
}

hipError_t knn_sparse_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, int k, int64_t* d_idx, double* d_d2, hipStream_t s) {
    if (n_q == 0) return hipSuccess;
    if (k < 1 || k > PCR_KNN_MAX_K || n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_q, st = (uint32_t)stride_floats;
    // (the block sizes of knn_query_launch, for its reasons)
    if (k == 1) hipLaunchKernelGGL((knn_sparse_kernel<1, 256>), dim3((n + 255) / 256), dim3(256), 0, s, v, d_q, n, st, k, d_idx, d_d2);
    else if (k <= 8) hipLaunchKernelGGL((knn_sparse_kernel<8, 256>), dim3((n + 255) / 256), dim3(256), 0, s, v, d_q, n, st, k, d_idx, d_d2);
    else if (k <= 16) hipLaunchKernelGGL((knn_sparse_kernel<16, 64>), dim3((n + 63) / 64), dim3(64), 0, s, v, d_q, n, st, k, d_idx, d_d2);
    else hipLaunchKernelGGL((knn_sparse_kernel<32, 64>), dim3((n + 63) / 64), dim3(64), 0, s, v, d_q, n, st, k, d_idx, d_d2);
    return hipGetLastError();
}

hipError_t radius_sparse_count_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, double radius, uint32_t* d_counts,
                                      unsigned long long* d_offsets, hipStream_t s) {
    if (n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_q;
    if (n)
        hipLaunchKernelGGL((radius_sparse_kernel<false>), dim3((n + 3) / 4), dim3(256), 0, s, v, d_q, n, (uint32_t)stride_floats, radius, radius * radius,
                           d_counts, (const unsigned long long*)nullptr, (int64_t*)nullptr, (double*)nullptr);
    return radius_scan_launch(d_counts, n_q, d_offsets, s);
}

hipError_t radius_sparse_fill_launch(const sw::View& v, const float* d_q, size_t n_q, size_t stride_floats, double radius, const unsigned long long* d_offsets,
                                     int64_t* d_idx, double* d_d2, hipStream_t s) {
    if (n_q == 0) return hipSuccess;
    if (n_q > 0xfffffff0ull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)n_q;
    hipLaunchKernelGGL((radius_sparse_kernel<true>), dim3((n + 3) / 4), dim3(256), 0, s, v, d_q, n, (uint32_t)stride_floats, radius, radius * radius,
                       (uint32_t*)nullptr, d_offsets, d_idx, d_d2);
    return hipGetLastError();
}

}  // namespace pcr
