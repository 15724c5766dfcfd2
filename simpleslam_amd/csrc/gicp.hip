// gicp.hip -- point-wise GICP scan-to-map on gfx950 (hand-written HIP).
//
// Kernels for fast_gicp::FastGICP (pclomp/src/fast_gicp_impl.hpp:103-237), the class FastVGICP derives from, under the same
// LsqRegistration loop (vgicp_opt.h):
//   update_correspondences   :120-153  serial there: a 1-NN of every transformed source point in a FLANN kd-tree, the gate on the
//      squared distance, (C_B + T C_A T^T)^-1 per pair
//   linearize                :156-211  H, b, error over the pairs
//   compute_error            :214-237  the error at a trial pose on the pairs of the last linearisation
//   -> gicp_lin_body<false> (update_correspondences + linearize in one pass) and <true> (compute_error of an LM trial pose on the
//      other correspondence buffer + the linearisation AT that pose), the sums through vgicp.hip's fixed-order reduction.
// The covariances of both clouds are vgicp.hip's (vgicp_cov_kernel / cov_search.hip); the search is ring_search.h's exact 1-NN in
// PCL's float metric, as the fitness score uses it.
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "small_math.h"
#include "vgicp_opt.h"
#include "ring_search.h"

namespace pcr {

static constexpr int kLinStride = 258;      // (vgicp.hip: the row stride of the block reduction)
static constexpr uint32_t kNoCorr = 0xffffffffu;

// the pair of source point i at pose T: the nearest target point of T a_i in float (ties on the lower original index), gated;
// then v[0..20] H (upper triangle), v[21..26] b, v[27] error.  The pair goes to corr_out / M_out.
__device__ __forceinline__ void gicp_lin_point(const GicpArgs& a, const Pose16& T, uint32_t i, double v[28], uint32_t* __restrict__ corr_out,
                                               double* __restrict__ M_out) {
    const float* sp = a.src + (size_t)i * a.src_stride;
    const float ax = sp[0], ay = sp[1], az = sp[2];
    uint32_t j = kNoCorr;
    float d2 = __uint_as_float(0x7f800000u);
    if (isfinite(ax) && isfinite(ay) && isfinite(az)) {
        // pcl::transformPointCloud with a Matrix4f (fitness_kernel's expression)
        const float qx = (float)T.m[0] * ax + (float)T.m[4] * ay + (float)T.m[8] * az + (float)T.m[12];
        const float qy = (float)T.m[1] * ax + (float)T.m[5] * ay + (float)T.m[9] * az + (float)T.m[13];
        const float qz = (float)T.m[2] * ax + (float)T.m[6] * ay + (float)T.m[10] * az + (float)T.m[14];
        KeyList<1> L;
        // (a nearest point at or beyond the gate is no correspondence: the search may stop there)
        ring_knn<1>(one_level(a.grid), qx, qy, qz, a.thr2, L);
        if (L.k[0] != ~0ull) {
            const float d = __uint_as_float((uint32_t)(L.k[0] >> 32));
            if (d < a.thr2) { j = (uint32_t)L.k[0]; d2 = d; }      // fast_gicp_impl.hpp:136
        }
    }
    corr_out[i] = j;
    if (a.d2_out) a.d2_out[i] = d2;
    if (j == kNoCorr) return;
    const double p[3] = {(double)ax, (double)ay, (double)az};
    double tp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) tp[r] = T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0;
    const float* bp = a.tgt + (size_t)j * a.tgt_stride;
    const double* cb = a.tgt_cov6 + (size_t)j * 6;
    const double* ca = a.src_cov6 + (size_t)i * 6;
    const double CA[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
    double RC[3][3], S[6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) RC[r][c] = T.m[r] * CA[0][c] + T.m[4 + r] * CA[1][c] + T.m[8 + r] * CA[2][c];
    int o = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) { S[o] = cb[o] + (RC[r][0] * T.m[c] + RC[r][1] * T.m[4 + c] + RC[r][2] * T.m[8 + c]); ++o; }
    double M6[6];
    inv3_sym(S, M6);   // (C_B + R C_A R^T)^-1: the 3 x 3 block of the reference's 4 x 4 inverse (fast_gicp_impl.hpp:146-150)
#pragma unroll
    for (int k = 0; k < 6; ++k) M_out[(size_t)i * 6 + k] = M6[k];
    const double M[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
    const double er[3] = {(double)bp[0] - tp[0], (double)bp[1] - tp[1], (double)bp[2] - tp[2]};
    double Me[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Me[r] = M[r][0] * er[0] + M[r][1] * er[1] + M[r][2] * er[2];
    // J = [skew(Tp) | -I]   fast_gicp_impl.hpp:188-190
    const double J[3][6] = {{0, -tp[2], tp[1], -1, 0, 0}, {tp[2], 0, -tp[0], 0, -1, 0}, {-tp[1], tp[0], 0, 0, 0, -1}};
    double MJ[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) MJ[r][c] = M[r][0] * J[0][c] + M[r][1] * J[1][c] + M[r][2] * J[2][c];
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[q++] = J[0][r] * MJ[0][c] + J[1][r] * MJ[1][c] + J[2][r] * MJ[2][c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = J[0][r] * Me[0] + J[1][r] * Me[1] + J[2][r] * Me[2];
    v[27] = er[0] * Me[0] + er[1] * Me[1] + er[2] * Me[2];
}

// compute_error (fast_gicp_impl.hpp:214-237) of one point: the pair and the Mahalanobis matrix of the LAST linearisation, new pose
__device__ __forceinline__ double gicp_err_point(const GicpArgs& a, const Pose16& T, uint32_t i) {
    const uint32_t j = a.corr[i];
    if (j == kNoCorr) return 0.0;
    const float* sp = a.src + (size_t)i * a.src_stride;
    const double p[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
    const float* bp = a.tgt + (size_t)j * a.tgt_stride;
    double er[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) er[r] = (double)bp[r] - (T.m[r] * p[0] + T.m[4 + r] * p[1] + T.m[8 + r] * p[2] + T.m[12 + r] * 1.0);
    const double* M6 = a.corr_M + (size_t)i * 6;
    const double Me0 = M6[0] * er[0] + M6[1] * er[1] + M6[2] * er[2], Me1 = M6[1] * er[0] + M6[3] * er[1] + M6[4] * er[2],
                 Me2 = M6[2] * er[0] + M6[4] * er[1] + M6[5] * er[2];
    return er[0] * Me0 + er[1] * Me1 + er[2] * Me2;
}

// kWithError = false: update_correspondences + linearize at T -- pairs to a.corr / a.corr_M, partial sums [0..27].
// kWithError = true: one pass for an LM trial pose T: [28] = compute_error(T) on the pairs of the last linearisation (a.corr / a.corr_M,
// read only) AND the linearisation AT T (pairs to a.corr_next / a.corr_M_next, sums [0..27]) -- what vgicp_lin_body does for VGICP, so
// that vg_opt::ctl_step and its parity rule serve both.  One source point per thread; the 28 or 29 sums leave through the same
// fixed-order LDS reduction into [block][32] rows: no atomics, bit-for-bit repeatable.
template <bool kWithError>
__device__ __forceinline__ void gicp_lin_body(const GicpArgs& a, const Pose16& T, double* sh /* [29][kLinStride] */, double* sh_sum /* [8][32] */) {
    constexpr int kRows = kWithError ? 29 : 28;
    const int tid = threadIdx.x, e = tid & 31, ch = tid >> 5;
    double acc = 0.0;
    for (uint32_t base = blockIdx.x * 256; base < a.n_src; base += gridDim.x * 256) {
        const uint32_t i = base + tid;
        double v[28];
#pragma unroll
        for (int k = 0; k < 28; ++k) v[k] = 0.0;
        double err = 0.0;
        if (i < a.n_src) {
            if (kWithError) {
                err = gicp_err_point(a, T, i);
                gicp_lin_point(a, T, i, v, a.corr_next, a.corr_M_next);
            } else {
                gicp_lin_point(a, T, i, v, a.corr, a.corr_M);
            }
        }
#pragma unroll
        for (int k = 0; k < 28; ++k) sh[k * kLinStride + tid] = v[k];
        if (kWithError) sh[28 * kLinStride + tid] = err;
        __syncthreads();
        if (e < kRows) {
            const double* row = sh + e * kLinStride + ch * 32;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) acc += row[k];
        }
        __syncthreads();
    }
    sh_sum[ch * 32 + e] = e < kRows ? acc : 0.0;
    __syncthreads();
    if (tid < 32) {
        double s = sh_sum[tid];
#pragma unroll
        for (int c = 1; c < 8; ++c) s += sh_sum[c * 32 + tid];
        a.partials[(size_t)blockIdx.x * 32 + tid] = s;
    }
}

template <bool kWithError>
__global__ __launch_bounds__(256) void gicp_linearize_kernel(const GicpArgs a, const Pose16 T) {
    __shared__ double sh[(kWithError ? 29 : 28) * kLinStride];
    __shared__ double sh_sum[8 * 32];
    gicp_lin_body<kWithError>(a, T, sh, sh_sum);
}

// ------------------------------------------------------------------------------
// Device-resident Levenberg-Marquardt loop: one launch per pass, whose prologue folds the rows of the previous launch and takes the
// optimiser's step -- vgicp_pass_pro_kernel's prologue restated for an unsharded target (no peer exchange, no region): the same
// fold order, the same vg_opt::ctl_step in every block, the same progress word and result block.
// ------------------------------------------------------------------------------
struct GicpProArgs {
    const double* rows_prev;     // [rows_prev_n][32]
    const VgCtl* ctl_prev;
    VgCtl* ctl_next;
    VgOut* out;
    double seq;
    uint32_t rows_prev_n;
    int32_t first;
};
static constexpr int kVgCtlWords = (int)((sizeof(VgCtl) + 3) / 4);
static_assert(sizeof(VgCtl) % 4 == 0, "VgCtl is copied word by word");

__global__ __launch_bounds__(256) void gicp_pass_pro_kernel(const GicpArgs a_in, const GicpProArgs pa) {
    __shared__ double sh[29 * kLinStride];
    __shared__ double sh_sum[8 * 32];
    __shared__ __attribute__((aligned(16))) uint32_t sh_ctl[kVgCtlWords];
    __shared__ double sh_sums[32];
    const int t = threadIdx.x;
    VgCtl* const c = reinterpret_cast<VgCtl*>(sh_ctl);
    // the state and the rows of the previous launch ([8 slices][32 components], 32 rows a thread per 256 rows; 512 rows beyond 65 536 source points)
    const int comp = t & 31, slice = t >> 5;
    double acc = 0.0;
    for (int w = t; w < kVgCtlWords; w += 256) sh_ctl[w] = reinterpret_cast<const uint32_t*>(pa.ctl_prev)[w];
    if (!pa.first)
        for (uint32_t r0 = 0; r0 < pa.rows_prev_n; r0 += 256) {
            double v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                const uint32_t row = r0 + (uint32_t)(slice + 8 * u);
                v[u] = row < pa.rows_prev_n ? pa.rows_prev[(size_t)row * 32 + comp] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 32; ++u) acc += v[u];
        }
    sh_sum[slice * 32 + comp] = acc;
    __syncthreads();
    if (c->done) {      // finished in an earlier launch: hand the state on to whatever is queued behind
        if (blockIdx.x == 0) for (int w = t; w < kVgCtlWords; w += 256) reinterpret_cast<uint32_t*>(pa.ctl_next)[w] = sh_ctl[w];
        return;
    }
    if (!pa.first) {
        if (t < 32) {
            double s = sh_sum[t];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += sh_sum[k * 32 + t];
            sh_sums[t] = s;
        }
        __syncthreads();
        if (t == 0) vg_opt::ctl_step(c, sh_sums);
        __syncthreads();
        if (blockIdx.x == 0) {
            for (int w = t; w < kVgCtlWords; w += 256) reinterpret_cast<uint32_t*>(pa.ctl_next)[w] = sh_ctl[w];
            if (t == 0) {
                VgOut* const out = pa.out;
                if (c->done) {
                    out->x0 = c->x0;
                    out->conv = c->conv; out->outer = c->outer; out->n_lin = c->n_lin; out->n_err = c->n_err; out->passes = c->passes;
                    out->roi_escapes = 0;
                    __threadfence_system();
                    __hip_atomic_store(&out->seq, pa.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    __hip_atomic_store(&out->progress, pa.seq * kProgressWindow + (double)c->passes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        if (c->done) return;
    }
    // the pose of this pass and the correspondence buffers, as scalars
    Pose16 T;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double v = c->xi.m[i];
        T.m[i] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    }
    const int kind = __builtin_amdgcn_readfirstlane(c->kind), parity = __builtin_amdgcn_readfirstlane(c->parity);
    GicpArgs a = a_in;
    if (parity) {
        a.corr = a_in.corr_next; a.corr_M = a_in.corr_M_next;
        a.corr_next = a_in.corr; a.corr_M_next = a_in.corr_M;
    }
    __syncthreads();      // (sh_sum is reused by the body)
    if (kind == kVgPassLinearize) gicp_lin_body<false>(a, T, sh, sh_sum);
    else gicp_lin_body<true>(a, T, sh, sh_sum);
}

// ---- host launchers ---------------------------------------------------------------
hipError_t gicp_launch_linearize(const GicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq) {
    const uint32_t nb = vgicp_blocks(a.n_src);
    hipLaunchKernelGGL(gicp_linearize_kernel<false>, dim3(nb), dim3(256), 0, s, a, T);
    return sum_partials_launch(a.partials, nb, d_out32, s, seq);
}

hipError_t gicp_launch_error(const GicpArgs& a, const Pose16& T, double* d_out32, hipStream_t s, double seq) {
    const uint32_t nb = vgicp_blocks(a.n_src);
    hipLaunchKernelGGL(gicp_linearize_kernel<true>, dim3(nb), dim3(256), 0, s, a, T);
    return sum_partials_launch(a.partials, nb, d_out32, s, seq);
}

// launch `index` of the device-resident loop: d_ctl2 = two VgCtl, d_rows2 = two buffers of 512 * 32 doubles (vgicp_launch_pass_pro's layout)
hipError_t gicp_launch_pass_pro(const GicpArgs& a_in, VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, hipStream_t s, double seq, int index) {
    const uint32_t nb = vgicp_blocks(a_in.n_src);
    GicpArgs a = a_in;
    a.partials = d_rows2 + (size_t)(index & 1) * 512 * 32;
    GicpProArgs pa;
    pa.rows_prev = d_rows2 + (size_t)((index + 1) & 1) * 512 * 32;
    pa.ctl_prev = index == 0 ? d_ctl2 : d_ctl2 + ((index + 1) & 1);
    pa.ctl_next = d_ctl2 + (index & 1);
    pa.out = d_out; pa.seq = seq; pa.rows_prev_n = nb; pa.first = index == 0 ? 1 : 0;
    hipLaunchKernelGGL(gicp_pass_pro_kernel, dim3(nb), dim3(256), 0, s, a, pa);
    return hipGetLastError();
}

}  // namespace pcr
