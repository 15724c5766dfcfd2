// liorf.hip -- LIO-SAM's surface scan-to-map on gfx950 (hand-written HIP): LioScan2map of the reference's test/comp/liorf_scan2map.cpp.
//
//   surfOptimization   :163-232  (OpenMP there: per scan point the float transform, a 5-NN in a FLANN kd-tree, a float plane fit)
//      -> liorf_point: the transform in pointAssociateToMap's expression, ring_search.h's exact 5-NN in PCL's float metric (ties on the
//         lower index), small_math.h's float column-pivoted QR, the weight, the row [d/droll, d/dpitch, d/dyaw, coeff | -intensity] of :306-324
//   LMOptimization     :248-383  (serial there: matAt * matA in float, cv::solve(DECOMP_QR), cv::eigen)
//      -> the rows' 21 + 6 products summed in double by lsq_pass.h's fixed-order reduction (a product of two floats is exact in double,
//         so this is the correctly rounded version of the float sums OpenCV takes in an order of its own), and lf_opt::ctl_step
//         (liorf_opt.h) in the prologue of the NEXT launch: the rounding to float, the float 6x6 QR solve, the step, the convergence
//         test, the rebuild of the float 4x4 -- one launch per iteration, no host round trip inside the loop.
// The plain per-lane search: no neighbour cache, no LDS-DMA fetch, no two-lane variant (those are loam.hip's).
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "small_math.h"
#include "liorf_opt.h"
#include "lsq_pass.h"
#include "ring_search.h"

namespace pcr {

static constexpr int kLfCtlWords = (int)(sizeof(LiorfCtl) / 4);
static_assert(sizeof(LiorfCtl) % 4 == 0, "LiorfCtl is copied word by word");

// surfOptimization of scan point i at the float 4x4 T (rows 0..2, row-major) + its row of LMOptimization from the angle matrices G:
// v[0..20] the upper triangle of row^T row, v[21..26] row^T (-intensity), v[27] 1 -- zeros when the point gives no row.
__device__ __forceinline__ void liorf_point(const LiorfArgs& a, const float T[12], const float G[27], uint32_t i, double v[28]) {
    const float* sp = a.src + (size_t)i * a.src_stride;
    const float px = sp[0], py = sp[1], pz = sp[2];
    bool keep = false;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, ci = 0.0f;
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
        // pointAssociateToMap (:147-149)
        const float qx = T[0] * px + T[1] * py + T[2] * pz + T[3];
        const float qy = T[4] * px + T[5] * py + T[6] * pz + T[7];
        const float qz = T[8] * px + T[9] * py + T[10] * pz + T[11];
        KeyList<5> L;
        // (a fifth neighbour at or beyond the gate gives no row: the search may stop a little beyond it)
        ring_knn<5>(one_level(a.grid), qx, qy, qz, (float)a.c.knn_max_sq * 1.001f, L);
        if (L.k[4] != ~0ull && (double)__uint_as_float((uint32_t)(L.k[4] >> 32)) < a.c.knn_max_sq) {      // pointSearchSqDis[4] < 1.0 (:186)
            float nb[5][3], A0[5][3], X[3];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float* t = a.tgt + (size_t)(uint32_t)L.k[j] * a.tgt_stride;
#pragma unroll
                for (int d = 0; d < 3; ++d) A0[j][d] = nb[j][d] = t[d];
            }
            plane_qr_solve_f(A0, X);      // matA0.colPivHouseholderQr().solve(matB0), matB0 = -1 (:193)
            float pa = X[0], pb = X[1], pc = X[2], pd = 1.0f;
            const float ps = sqrtf(pa * pa + pb * pb + pc * pc);
            pa /= ps; pb /= ps; pc /= ps; pd /= ps;
            bool valid = true;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if ((double)fabsf(pa * nb[j][0] + pb * nb[j][1] + pc * nb[j][2] + pd) > a.c.plane_thresh) valid = false;      // (:205-207)
            if (valid) {
                const float pd2 = pa * qx + pb * qy + pc * qz + pd;
                // float s = 1 - 0.9 * fabs(pd2) / sqrt(sqrt(|pointOri|^2)): the roots in float, the product and the quotient in double (:216)
                const float s = (float)(1.0 - 0.9 * (double)fabsf(pd2) / (double)sqrtf(sqrtf(px * px + py * py + pz * pz)));
                if ((double)s > a.c.point_thresh) {      // (:224)
                    keep = true;
                    cx = s * pa; cy = s * pb; cz = s * pc; ci = s * pd2;
                }
            }
        }
    }
    if (a.kept_out) {
        a.kept_out[i] = keep ? 1 : 0;
        float* co = a.coeff_out + (size_t)i * 4;
        co[0] = cx; co[1] = cy; co[2] = cz; co[3] = ci;
    }
    if (!keep) return;
    // the angular entries: coeff . (G_a p) for a = roll, pitch, yaw (liorf_opt.h: row_matrices), each sum left to right
    float ang[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* g = G + 9 * k;
        const float u0 = g[0] * px + g[1] * py + g[2] * pz, u1 = g[3] * px + g[4] * py + g[5] * pz, u2 = g[6] * px + g[7] * py + g[8] * pz;
        ang[k] = u0 * cx + u1 * cy + u2 * cz;
    }
    const double row[6] = {(double)ang[0], (double)ang[1], (double)ang[2], (double)cx, (double)cy, (double)cz};
    const double rhs = (double)(-ci);
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[q++] = row[r] * row[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = row[r] * rhs;
    v[27] = 1.0;
}

// lsq_pass.h's pass over the scan with liorf's per-point function (the pose argument of that interface is not used: the float 4x4 is the state's)
struct LiorfPass {
    const LiorfArgs& a;
    const float* T;
    const float* G;
    __device__ __forceinline__ void lin(const Pose16&, uint32_t i, double v[28], bool) const { liorf_point(a, T, G, i, v); }
    __device__ __forceinline__ double err(const Pose16&, uint32_t) const { return 0.0; }
};

struct LiorfProArgs {
    const double* rows_prev;     // [rows_prev_n][32]
    const LiorfCtl* ctl_prev;
    LiorfCtl* ctl_next;
    LiorfOut* out;
    double seq;
    uint32_t rows_prev_n;
    int32_t first;               // launch 0: the state starts from a.six0
    int32_t once;                // pcr_liorf_linearize: one linearisation, whatever liorf_iters says
};

// A launch of the device-resident loop.  Prologue, in every block on the same numbers: the fold of the previous launch's rows and the
// optimiser's step (launch 0: the initial state); block 0 hands the state on and writes the result or the progress word.  Then, unless
// the loop has ended, the linearisation at the state's six numbers.
__global__ __launch_bounds__(256) void liorf_iterate_kernel(const LiorfArgs a, const LiorfProArgs pa) {
    __shared__ double sh[28 * kLinStride];
    __shared__ double sh_sum[8 * 32];
    __shared__ double sh_sums[32];
    __shared__ __attribute__((aligned(16))) uint32_t sh_ctl[kLfCtlWords];
    const int t = threadIdx.x, comp = t & 31, slice = t >> 5;
    LiorfCtl* const c = reinterpret_cast<LiorfCtl*>(sh_ctl);
    if (pa.first) {
        if (t == 0) lf_opt::ctl_init(c, a.six0, pa.once ? 1 : a.c.iters, a.c.file_row != 0);
        __syncthreads();
    } else {
        const double acc = lsq_fold_rows<false>(pa.rows_prev, pa.rows_prev_n, 0, nullptr, nullptr);
        if (t < kLfCtlWords) sh_ctl[t] = reinterpret_cast<const uint32_t*>(pa.ctl_prev)[t];
        sh_sum[slice * 32 + comp] = acc;
        __syncthreads();
        if (c->done) {      // finished in an earlier launch: hand the state on to whatever is queued behind
            if (blockIdx.x == 0 && t < kLfCtlWords) reinterpret_cast<uint32_t*>(pa.ctl_next)[t] = sh_ctl[t];
            return;
        }
        if (t < 32) {
            double s = sh_sum[t];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += sh_sum[k * 32 + t];
            sh_sums[t] = s;
        }
        __syncthreads();
        if (t == 0) lf_opt::ctl_step(c, sh_sums, a.c, blockIdx.x == 0 ? a.trace : nullptr);
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        if (t < kLfCtlWords) reinterpret_cast<uint32_t*>(pa.ctl_next)[t] = sh_ctl[t];
        if (t == 0 && pa.out) {
            LiorfOut* const out = pa.out;
            if (c->done) {
#pragma unroll
                for (int i = 0; i < 6; ++i) out->six[i] = c->six[i];
                out->converged = c->converged; out->iters_run = c->iters_run; out->degenerate = c->degenerate;
                out->rows_last = c->rows_last; out->passes = c->passes;
                __threadfence_system();
                __hip_atomic_store(&out->seq, pa.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                __hip_atomic_store(&out->progress, pa.seq * kProgressWindow + (double)c->passes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    if (c->done) return;
    // the float 4x4 and the rows' angle matrices, as scalars
    float T[12], G[27];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c->T[i])));
#pragma unroll
    for (int i = 0; i < 27; ++i) G[i] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c->G[i])));
    const LiorfPass m{a, T, G};
    const Pose16 unused{};
    __syncthreads();      // (sh_sum is reused by the body)
    lsq_lin_body<false>(m, unused, a.n_src, a.partials, sh, sh_sum);
}

// ---- host launchers ---------------------------------------------------------------
uint32_t liorf_blocks(uint32_t n_src) { return vgicp_blocks(n_src); }

static LiorfProArgs liorf_pro_args(LiorfCtl* d_ctl2, double* d_rows2, LiorfOut* d_out, double seq, int index, uint32_t nb) {
    LiorfProArgs pa;
    pa.rows_prev = lsq_rows(d_rows2, index + 1);
    pa.ctl_prev = d_ctl2 + ((index + 1) & 1);
    pa.ctl_next = d_ctl2 + (index & 1);
    pa.out = d_out; pa.seq = seq; pa.rows_prev_n = nb; pa.first = index == 0 ? 1 : 0; pa.once = 0;
    return pa;
}

hipError_t liorf_launch_pass(const LiorfArgs& a_in, LiorfCtl* d_ctl2, double* d_rows2, LiorfOut* d_out, hipStream_t s, double seq, int index) {
    const uint32_t nb = liorf_blocks(a_in.n_src);
    LiorfArgs a = a_in;
    a.partials = lsq_rows(d_rows2, index);
    const LiorfProArgs pa = liorf_pro_args(d_ctl2, d_rows2, d_out, seq, index, nb);
    hipLaunchKernelGGL(liorf_iterate_kernel, dim3(nb), dim3(256), 0, s, a, pa);
    return hipGetLastError();
}

hipError_t liorf_launch_linearize(const LiorfArgs& a_in, LiorfCtl* d_ctl2, double* d_rows2, LiorfOut* d_out, double* d_out32, hipStream_t s, double seq) {
    (void)d_out;
    const uint32_t nb = liorf_blocks(a_in.n_src);
    LiorfArgs a = a_in;
    a.partials = lsq_rows(d_rows2, 0);
    LiorfProArgs pa = liorf_pro_args(d_ctl2, d_rows2, nullptr, seq, 0, nb);
    pa.once = 1;
    hipLaunchKernelGGL(liorf_iterate_kernel, dim3(nb), dim3(256), 0, s, a, pa);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sum_partials_launch(a.partials, nb, d_out32, s, seq);
}

}  // namespace pcr
