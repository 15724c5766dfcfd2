// gicp.hip -- point-wise GICP scan-to-map on gfx950 (hand-written HIP).
//
// Kernels for fast_gicp::FastGICP (pclomp/src/fast_gicp_impl.hpp:103-237), the class FastVGICP derives from, under the same
// LsqRegistration loop (vgicp_opt.h):
//   update_correspondences   :120-153  serial there: a 1-NN of every transformed source point in a FLANN kd-tree, the gate on the
//      squared distance, (C_B + T C_A T^T)^-1 per pair
//   linearize                :156-211  H, b, error over the pairs
//   compute_error            :214-237  the error at a trial pose on the pairs of the last linearisation
//   -> gicp_lin_point (update_correspondences + linearize of one source point) and gicp_err_point (compute_error of one point), the
//      two functions VGICP's pass does not have.  The pass around them -- the fixed-order reduction of the sums, the trial pass that
//      also linearises at its pose, the device-resident loop's prologue -- is lsq_pass.h's, shared with vgicp.hip.
// The covariances of both clouds are vgicp.hip's (vgicp_cov_kernel / cov_search.hip); the search is ring_search.h's exact 1-NN in
// PCL's float metric, as the fitness score uses it.
#include <float.h>
#include <math.h>
#include <string.h>

#include "pcr_internal.h"
#include "small_math.h"
#include "vgicp_opt.h"
#include "lsq_pass.h"
#include "ring_search.h"

namespace pcr {

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

// The pass of lsq_pass.h over GICP's point pairs
struct GicpPass {
    const GicpArgs& a;
    __device__ __forceinline__ void lin(const Pose16& T, uint32_t i, double v[28], bool to_next) const {
        gicp_lin_point(a, T, i, v, to_next ? a.corr_next : a.corr, to_next ? a.corr_M_next : a.corr_M);
    }
    __device__ __forceinline__ double err(const Pose16& T, uint32_t i) const { return gicp_err_point(a, T, i); }
};

template <bool kWithError>
__global__ __launch_bounds__(256) void gicp_linearize_kernel(const GicpArgs a, const Pose16 T) {
    __shared__ double sh[(kWithError ? 29 : 28) * kLinStride];
    __shared__ double sh_sum[8 * 32];
    lsq_lin_body<kWithError>(GicpPass{a}, T, a.n_src, a.partials, sh, sh_sum);
}

// a launch of the device-resident Levenberg-Marquardt loop (lsq_pass.h), of an unsharded target: no peer exchange, no region
__global__ __launch_bounds__(256) void gicp_pass_pro_kernel(const GicpArgs a, const LsqProArgs pa) {
    __shared__ double sh[29 * kLinStride];
    __shared__ double sh_sum[8 * 32];
    __shared__ __attribute__((aligned(16))) uint32_t sh_ctl[kVgCtlWords];
    __shared__ double sh_sums[32];
    lsq_pass<false, GicpPass>(a, pa, nullptr, sh, sh_sum, sh_ctl, sh_sums);
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

// launch `index` of the device-resident loop (lsq_pass.h: lsq_pro_args)
hipError_t gicp_launch_pass_pro(const GicpArgs& a_in, VgCtl* d_ctl2, double* d_rows2, VgOut* d_out, hipStream_t s, double seq, int index) {
    const uint32_t nb = vgicp_blocks(a_in.n_src);
    GicpArgs a = a_in;
    a.partials = lsq_rows(d_rows2, index);
    const LsqProArgs pa = lsq_pro_args(d_ctl2, d_rows2, d_out, seq, index, nb);
    hipLaunchKernelGGL(gicp_pass_pro_kernel, dim3(nb), dim3(256), 0, s, a, pa);
    return hipGetLastError();
}

}  // namespace pcr
