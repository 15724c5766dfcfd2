// nb_list.h -- the k-NN list of the exact queries (knn_query.hip on the dense index, sparse_index.hip on the sparse one): K (d2, index) pairs in
// registers, ascending by (d2, index), kept by an unrolled insertion.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcr {

template <int K>
struct NbList {
    double d[K];
    uint32_t i[K];
};

template <int K>
__device__ __forceinline__ void nb_insert(NbList<K>& L, double d, uint32_t idx) {
    bool c[K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = d < L.d[i] || (d == L.d[i] && idx < L.i[i]);
#pragma unroll
    for (int i = K - 1; i >= 1; --i) {
        L.d[i] = c[i - 1] ? L.d[i - 1] : (c[i] ? d : L.d[i]);
        L.i[i] = c[i - 1] ? L.i[i - 1] : (c[i] ? idx : L.i[i]);
    }
    L.d[0] = c[0] ? d : L.d[0];
    L.i[0] = c[0] ? idx : L.i[0];
}

template <int K>
__device__ __forceinline__ void nb_scan_run(const float4* __restrict__ pts, uint32_t s, uint32_t e, double qx, double qy, double qz, NbList<K>& L) {
    // four candidates per step, their loads issued together (ring_search.h: ring_scan_run)
    for (uint32_t j = s; j < e; j += 4) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[j + u < e ? j + u : j];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = qx - (double)p[u].x, dy = qy - (double)p[u].y, dz = qz - (double)p[u].z;
            double d = dx * dx;
            d += dy * dy;
            d += dz * dz;
            const uint32_t idx = __float_as_uint(p[u].w);
            if (j + u < e && (d < L.d[K - 1] || (d == L.d[K - 1] && idx < L.i[K - 1]))) nb_insert<K>(L, d, idx);
        }
    }
}

}  // namespace pcr
