// kf_rank.h -- the arithmetic of the key-frame ranking by distance (pcr_kf_rank_near_host, pcr_map_rank_near), for device and host: the squared
// distance in the order pcr_frontend_step's step 6 forms it, the test for a usable position, the total order (d2, index) and the k-best list
// that the kernel keeps per lane and the host keeps per query.  No math library and no HIP call: a host compiler takes it as it is
// (-ffp-contract=off there as in the library: every operation is rounded on its own).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KFR_HD __host__ __device__
#else
#define KFR_HD
#endif

namespace pcr {
namespace kfr {

constexpr int kMaxK = 8;
constexpr int kNone = 0x7fffffff;                     // the index of a free slot of a list: it sorts behind every key frame
constexpr double kTailD2 = 1.7976931348623157e308;    // DBL_MAX: what a free slot leaves in the caller's d2

// x - x is 0 for every finite x and NaN for an infinity or a NaN
KFR_HD inline bool finite3(double x, double y, double z) { return (x - x == 0.0) && (y - y == 0.0) && (z - z == 0.0); }

// (dx dx + dy dy) + dz dz, five roundings (MapManager.cpp:141-143 as pcr_frontend_step has it)
KFR_HD inline double dist2(double qx, double qy, double qz, double cx, double cy, double cz) {
    const double dx = cx - qx, dy = cy - qy, dz = cz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// The first coordinate of a position as the ranking reads it: NaN when any coordinate is not finite, so that dist2 is NaN and no
// comparison with the radius holds.  (An infinite coordinate alone would give d2 = inf, which a radius whose square overflows admits.)
KFR_HD inline double usable_x(double x, double y, double z) { return finite3(x, y, z) ? x : __builtin_nan(""); }

KFR_HD inline bool before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// The k best of what was offered, ascending by (d2, index); free slots hold (+inf, kNone).  K is a template parameter and every loop has
// constant bounds: the slots stay in registers (a dynamically indexed private array would go to scratch).
template <int K>
struct Best {
    double d[K];
    int i[K];
    KFR_HD void clear() {
#pragma unroll
        for (int s = 0; s < K; ++s) { d[s] = __builtin_inf(); i[s] = kNone; }
    }
    // one pass from the back: every slot the newcomer comes before moves one down, the newcomer takes its place
    KFR_HD void offer(double nd, int ni) {
        if (!before(nd, ni, d[K - 1], i[K - 1])) return;
#pragma unroll
        for (int s = K - 1; s >= 0; --s) {
            if (before(nd, ni, d[s], i[s])) {
                if (s + 1 < K) { d[s + 1] = d[s]; i[s + 1] = i[s]; }
                d[s] = nd; i[s] = ni;
            }
        }
    }
    // the head leaves, the rest moves up
    KFR_HD void pop() {
#pragma unroll
        for (int s = 0; s + 1 < K; ++s) { d[s] = d[s + 1]; i[s] = i[s + 1]; }
        d[K - 1] = __builtin_inf(); i[K - 1] = kNone;
    }
};

// One query on the host, the definition: candidates [0, lim) of the arrays, the k best into row (k entries of idx and d2)
template <int K>
inline void rank_row(const double* x, const double* y, const double* z, long long lim, double qx, double qy, double qz, double r2, int64_t* idx, double* d2) {
    Best<K> b;
    b.clear();
    const double ux = usable_x(qx, qy, qz);
    for (long long c = 0; c < lim; ++c) {
        const double d = dist2(ux, qy, qz, usable_x(x[c], y[c], z[c]), y[c], z[c]);
        if (d <= r2) b.offer(d, (int)c);
    }
    for (int s = 0; s < K; ++s) {
        idx[s] = b.i[s] == kNone ? -1 : b.i[s];
        d2[s] = b.i[s] == kNone ? kTailD2 : b.d[s];
    }
}

}  // namespace kfr
}  // namespace pcr
