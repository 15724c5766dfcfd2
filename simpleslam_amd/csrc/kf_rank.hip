// kf_rank.hip -- key frames ranked by distance, the loop detector the reference declares and leaves empty (backend/DistContext.hpp: a kd-tree over
// key-frame positions): for every query key frame q the k nearest key frames of [0, q - num_exclude_recent) within a radius.  On a loaded map that
// is all pairs of tens of thousands of positions, so it runs on the device next to sc_rank_stored_kernel and in its shape: a tile of queries in LDS,
// the candidates streamed past them in tiles, a private k-best per lane, a merge in a fixed order, no atomics.  The arithmetic is kf_rank.h's,
// which pcr_kf_rank_near_host runs on the host: the two agree bit for bit.  DESIGN 4.18.

#include <cmath>
#include <string>
#include <vector>

#include "pcr_internal.h"
#include "kf_rank.h"

using namespace pcr;

namespace {

// A block holds kTileQ queries; kLanesQ lanes share one query (a wave serves four) and split every candidate tile between them: lane s of a query
// takes the tile's candidates s, s + kLanesQ, ... in ascending order.  A staged candidate serves kTileQ pairs.
constexpr int kTileQ = 16, kLanesQ = 16, kTileC = 256, kThreads = kTileQ * kLanesQ;
static_assert(kThreads == kTileC && 64 % kLanesQ == 0, "one staged candidate per thread; a query's lanes lie in one wave");

// Query q = first + blockIdx.x * kTileQ + j against candidates [0, q - excl): the k best by (d2, index) with d2 <= r2 into row q - first.
// lim_last, the last query's limit, bounds the stream for the whole block (block-uniform: the barriers are met by every thread); it is at most
// first + count - 1 < n, so every position read lies inside the arrays.  After the stream the kLanesQ lists of a query are merged in K rounds:
// each round the smallest head by (d2, index) among the lanes -- an xor butterfly inside the query's lanes -- is written and leaves its list.
// A candidate stands in one list and (d2, index) is a total order, so the result depends on no schedule.
template <int K>
__global__ __launch_bounds__(kThreads) void kf_rank_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                           unsigned int first, unsigned int count, int excl, double r2, long long* __restrict__ idx,
                                                           double* __restrict__ d2) {
    __shared__ double s_q[3][kTileQ];
    __shared__ double s_c[3][kTileC];
    const int tid = threadIdx.x, j = tid / kLanesQ, s = tid % kLanesQ;
    const unsigned int q0 = first + blockIdx.x * kTileQ;
    const int nq = (int)(first + count - q0 < (unsigned int)kTileQ ? first + count - q0 : (unsigned int)kTileQ);
    if (tid < kTileQ) {
        const bool live = tid < nq;
        const double px = live ? x[q0 + tid] : 0.0, py = live ? y[q0 + tid] : 0.0, pz = live ? z[q0 + tid] : 0.0;
        s_q[0][tid] = kfr::usable_x(px, py, pz); s_q[1][tid] = py; s_q[2][tid] = pz;
    }
    const long long lim_last = (long long)(q0 + nq - 1) - excl;
    __syncthreads();
    const double qx = s_q[0][j], qy = s_q[1][j], qz = s_q[2][j];
    const long long lim = j < nq ? (long long)(q0 + j) - excl : 0;      // this query's candidates: [0, lim)
    kfr::Best<K> best;
    best.clear();
    for (long long c0 = 0; c0 < lim_last; c0 += kTileC) {
        const long long c = c0 + tid;
        const bool in = c < lim_last;
        const double px = in ? x[c] : 0.0, py = in ? y[c] : 0.0, pz = in ? z[c] : 0.0;
        s_c[0][tid] = kfr::usable_x(px, py, pz); s_c[1][tid] = py; s_c[2][tid] = pz;
        __syncthreads();
#pragma unroll 4
        for (int t = s; t < kTileC; t += kLanesQ) {
            const long long cc = c0 + t;
            if (cc < lim) {
                const double d = kfr::dist2(qx, qy, qz, s_c[0][t], s_c[1][t], s_c[2][t]);
                if (d <= r2) best.offer(d, (int)cc);
            }
        }
        __syncthreads();
    }
    const size_t out = (size_t)(q0 + j - first) * K;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        double wd = best.d[0];
        int wi = best.i[0];
#pragma unroll
        for (int m = 1; m < kLanesQ; m <<= 1) {
            const double od = __shfl_xor(wd, m);
            const int oi = __shfl_xor(wi, m);
            if (kfr::before(od, oi, wd, wi)) { wd = od; wi = oi; }
        }
        if (wi != kfr::kNone && wi == best.i[0]) best.pop();
        if (s == 0 && j < nq) {
            idx[out + r] = wi == kfr::kNone ? -1 : wi;
            d2[out + r] = wi == kfr::kNone ? kfr::kTailD2 : wd;
        }
    }
}

template <int K>
void launch_rank(const double* x, const double* y, const double* z, size_t first, size_t count, int excl, double r2, long long* idx, double* d2) {
    const unsigned int blocks = (unsigned int)((count + kTileQ - 1) / kTileQ);
    hipLaunchKernelGGL(kf_rank_kernel<K>, dim3(blocks), dim3(kThreads), 0, 0, x, y, z, (unsigned int)first, (unsigned int)count, excl, r2, idx, d2);
}

template <int K>
void host_rank(const double* x, const double* y, const double* z, size_t first, size_t count, int excl, double r2, int64_t* idx, double* d2) {
    for (size_t q = first; q < first + count; ++q)
        kfr::rank_row<K>(x, y, z, (long long)q - excl, x[q], y[q], z[q], r2, idx + (q - first) * K, d2 + (q - first) * K);
}

#define KFR_DISPATCH(k, fn, ...)                                                                                       \
    switch (k) {                                                                                                       \
        case 1: fn<1>(__VA_ARGS__); break;  case 2: fn<2>(__VA_ARGS__); break;  case 3: fn<3>(__VA_ARGS__); break;     \
        case 4: fn<4>(__VA_ARGS__); break;  case 5: fn<5>(__VA_ARGS__); break;  case 6: fn<6>(__VA_ARGS__); break;     \
        case 7: fn<7>(__VA_ARGS__); break;  default: fn<8>(__VA_ARGS__); break;                                        \
    }

// what both entry points refuse, "" when the arguments are in order
std::string refusal(size_t n, size_t first, size_t count, int num_exclude_recent, double radius, int k, const int64_t* idx, const double* d2) {
    if (k < 1 || k > kfr::kMaxK) return "k must be 1..8, not " + std::to_string(k);
    if (!(radius >= 0.0) || !std::isfinite(radius)) return "radius must be finite and not negative";
    if (num_exclude_recent < 0) return "num_exclude_recent must not be negative";
    if (first > n || count > n - first) return "first + count = " + std::to_string(first) + " + " + std::to_string(count) + " exceeds the " + std::to_string(n) + " key frames";
    if (n > 0x7fffff00ull) return "too many key frames";
    if (count > 0 && !idx) return "idx is NULL";
    if (count > 0 && !d2) return "d2 is NULL";
    return "";
}

}  // namespace

extern "C" {

int pcr_kf_rank_near_host(const double* xyz, size_t n, size_t first, size_t count, int num_exclude_recent, double radius, int k, int64_t* idx, double* d2) {
    if (!refusal(n, first, count, num_exclude_recent, radius, k, idx, d2).empty()) return 1;
    if (count == 0) return 0;
    if (!xyz) return 1;
    const size_t np = first + count;
    std::vector<double> x(np), y(np), z(np);
    for (size_t i = 0; i < np; ++i) { x[i] = xyz[3 * i]; y[i] = xyz[3 * i + 1]; z[i] = xyz[3 * i + 2]; }
    KFR_DISPATCH(k, host_rank, x.data(), y.data(), z.data(), first, count, num_exclude_recent, radius * radius, idx, d2);
    return 0;
}

int pcr_map_rank_near(const pcr_map* m, size_t first, size_t count, int num_exclude_recent, double radius, int k, int64_t* idx, double* d2) {
    if (!m) return 1;
    size_t n = 0;
    if (pcr_map_keyframes(m, &n)) return 1;      // (a view whose parent is gone: the message is set)
    const std::string why = refusal(n, first, count, num_exclude_recent, radius, k, idx, d2);
    if (!why.empty()) return map_set_error(m, "pcr_map_rank_near: " + why);
    map_set_error(m, "");
    if (count == 0) return 0;
#define R_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return map_set_error(m, std::string("pcr_map_rank_near: " #x ": ") + hipGetErrorString(_e)); } while (0)
    // the positions of key frames [0, first + count) from the poses the store keeps on the host, as three arrays: 24 B per key frame, once per call
    const size_t np = first + count, rows = count * (size_t)k;
    std::vector<double> pos(3 * np);
    for (size_t i = 0; i < np; ++i) {
        double pose[16];
        size_t pts = 0;
        (void)pcr_map_keyframe(m, i, &pts, nullptr, pose);
        pos[i] = pose[12]; pos[np + i] = pose[13]; pos[2 * np + i] = pose[14];
    }
    R_TRY(hipSetDevice(map_device(m)));
    const size_t bytes = (3 * np + rows) * sizeof(double) + rows * sizeof(long long);
    double* d_pos = static_cast<double*>(map_scratch(m, bytes));
    if (!d_pos) return map_set_error(m, "pcr_map_rank_near: no device memory for " + std::to_string(bytes) + " bytes");
    double* d_d2 = d_pos + 3 * np;
    long long* d_idx = reinterpret_cast<long long*>(d_d2 + rows);
    R_TRY(hipMemcpy(d_pos, pos.data(), 3 * np * sizeof(double), hipMemcpyHostToDevice));
    KFR_DISPATCH(k, launch_rank, d_pos, d_pos + np, d_pos + 2 * np, first, count, num_exclude_recent, radius * radius, d_idx, d_d2);
    R_TRY(hipGetLastError());
    // into scratch first: a failed copy must leave the caller's arrays as they were
    std::vector<double> h_d2(rows);
    std::vector<long long> h_idx(rows);
    R_TRY(hipMemcpy(h_d2.data(), d_d2, rows * sizeof(double), hipMemcpyDeviceToHost));
    R_TRY(hipMemcpy(h_idx.data(), d_idx, rows * sizeof(long long), hipMemcpyDeviceToHost));
#undef R_TRY
    for (size_t i = 0; i < rows; ++i) { d2[i] = h_d2[i]; idx[i] = h_idx[i]; }
    return 0;
}

}  // extern "C"
