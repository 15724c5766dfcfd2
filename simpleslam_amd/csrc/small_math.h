// small_math.h -- tiny f64 linear-algebra routines shared by device kernels and host drivers.
// Restated from the Eigen calls of the reference (citations at each routine).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pcr {

// ------------------------------------------------------------------------------
// small f64 routines, single lane
// ------------------------------------------------------------------------------

// Eigen::LDLT<Matrix6d> (lower, diagonal pivoting) restated; M: full symmetric 6x6 row-major.
// Fully unrolled with static indices (pivot swaps are `if (p == pp)` over the static candidates)
// so the factor lives in registers: the single solving lane never touches scratch memory.
__host__ __device__ inline void ldlt6_solve(const double* M, const double* rhs, double* x) {
    double m[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) m[i][j] = (j <= i) ? M[i * 6 + j] : 0.0;
    }
    int tr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int p = k; double big = fabs(m[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) if (fabs(m[i][i]) > big) { big = fabs(m[i][i]); p = i; }
        tr[k] = p;
#pragma unroll
        for (int pp = k + 1; pp < 6; ++pp) {
            if (p == pp) {
#pragma unroll
                for (int j = 0; j < k; ++j) { const double t = m[k][j]; m[k][j] = m[pp][j]; m[pp][j] = t; }
#pragma unroll
                for (int i = pp + 1; i < 6; ++i) { const double t = m[i][k]; m[i][k] = m[i][pp]; m[i][pp] = t; }
#pragma unroll
                for (int i = k + 1; i < pp; ++i) { const double t = m[i][k]; m[i][k] = m[pp][i]; m[pp][i] = t; }
                const double t = m[k][k]; m[k][k] = m[pp][pp]; m[pp][pp] = t;
            }
        }
        if (k > 0) {
            double temp[6];
#pragma unroll
            for (int j = 0; j < k; ++j) temp[j] = m[j][j] * m[k][j];
            double s = 0;
#pragma unroll
            for (int j = 0; j < k; ++j) s += m[k][j] * temp[j];
            m[k][k] -= s;
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                double s2 = 0;
#pragma unroll
                for (int j = 0; j < k; ++j) s2 += m[i][j] * temp[j];
                m[i][k] -= s2;
            }
        }
        const double piv = m[k][k];
        if (fabs(piv) > 0.0) {
#pragma unroll
            for (int i = k + 1; i < 6; ++i) m[i][k] /= piv;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = rhs[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int pp = k + 1; pp < 6; ++pp) if (tr[k] == pp) { const double t = y[k]; y[k] = y[pp]; y[pp] = t; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) y[i] -= m[i][j] * y[j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = (fabs(m[i][i]) > 2.2250738585072014e-308) ? y[i] / m[i][i] : 0.0;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
#pragma unroll
        for (int j = i + 1; j < 6; ++j) y[i] -= m[j][i] * y[j];
    }
#pragma unroll
    for (int k = 5; k >= 0; --k) {
#pragma unroll
        for (int pp = k + 1; pp < 6; ++pp) if (tr[k] == pp) { const double t = y[k]; y[k] = y[pp]; y[pp] = t; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = y[i];
}

// manifolds::exp(V6) (manifolds.hpp:33-60): k = [rho; omega], T column-major.
__host__ __device__ inline void se3_exp(const double* k, double* T) {
    const double* p = k; const double* w = k + 3;
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    const double t = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (t < 1e-6) { T[12] = p[0]; T[13] = p[1]; T[14] = p[2]; return; }
    const double a[3] = {w[0] / t, w[1] / t, w[2] / t};
    const double ct = cos(t), st = sin(t);
    const double ah[3][3] = {{0, -a[2], a[1]}, {a[2], 0, -a[0]}, {-a[1], a[0], 0}};
    double V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double I = (i == j) ? 1.0 : 0.0, aa = a[i] * a[j];
            T[j * 4 + i] = ct * I + (1.0 - ct) * aa + st * ah[i][j];
            V[i][j] = st / t * I + (1.0 - st / t) * aa + ((1 - ct) / t) * ah[i][j];
        }
    for (int i = 0; i < 3; ++i) T[12 + i] = V[i][0] * p[0] + V[i][1] * p[1] + V[i][2] * p[2];
}

// trans::T2SE3 (trans.hpp:54-65): R <- Quaternion(R).normalized().toRotationMatrix().
__host__ __device__ inline void t2se3(double* T) {
#define M_(i, j) T[(j) * 4 + (i)]
    double q[4];
    double t = M_(0, 0) + M_(1, 1) + M_(2, 2);
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (M_(2, 1) - M_(1, 2)) * t; q[1] = (M_(0, 2) - M_(2, 0)) * t; q[2] = (M_(1, 0) - M_(0, 1)) * t;
    } else {
        int i = 0;
        if (M_(1, 1) > M_(0, 0)) i = 1;
        if (M_(2, 2) > M_(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(M_(i, i) - M_(j, j) - M_(k, k) + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (M_(k, j) - M_(j, k)) * t;
        q[j] = (M_(j, i) + M_(i, j)) * t;
        q[k] = (M_(k, i) + M_(i, k)) * t;
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                 tyz = tz * y, tzz = tz * z;
    M_(0, 0) = 1 - (tyy + tzz); M_(0, 1) = txy - twz; M_(0, 2) = txz + twy;
    M_(1, 0) = txy + twz; M_(1, 1) = 1 - (txx + tzz); M_(1, 2) = tyz - twx;
    M_(2, 0) = txz - twy; M_(2, 1) = tyz + twx; M_(2, 2) = 1 - (txx + tyy);
#undef M_
}


// inverse of a symmetric 3x3 (xx xy xz yy yz zz) by cofactors: the Mahalanobis matrices of VGICP and GICP (vgicp.hip, gicp.hip)
__host__ __device__ __forceinline__ void inv3_sym(const double S[6], double M[6]) {
    const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5];
    const double A = d * f - e * e, B = c * e - b * f, Cc = b * e - c * d;
    const double det = a * A + b * B + c * Cc;
    const double id = 1.0 / det;
    M[0] = A * id; M[1] = B * id; M[2] = Cc * id;
    M[3] = (a * f - c * c) * id; M[4] = (b * c - a * e) * id; M[5] = (a * d - b * b) * id;
}

// ------------------------------------------------------------------------------
// small f32 routines, single lane (liorf.hip, liorf_opt.h): all indices static, so everything stays in registers
// ------------------------------------------------------------------------------

// plane fit: Eigen::ColPivHouseholderQR<Matrix<float,5,3>>::solve(-1) restated (liorf_scan2map.cpp:193), the float sibling of
// loam.hip's plane_qr_solve: the same steps in the same order, with float's epsilon, sqrt(epsilon) and smallest normal number.
__host__ __device__ __forceinline__ void plane_qr_solve_f(float a[5][3], float x[3]) {
    float c[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
    int perm[3] = {0, 1, 2};
    float tau[3] = {0, 0, 0};
    float nu[3], nd[3];
    float maxn = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float s = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) s += a[i][j] * a[i][j];
        nd[j] = nu[j] = sqrtf(s);
        if (nu[j] > maxn) maxn = nu[j];
    }
    const float eps = 1.1920928955078125e-07f;
    const float thr_helper = (maxn * eps) * (maxn * eps) / 5.0f;
    const float downdate_thr = 3.4526698300124393e-04f;  // sqrt(eps)
    int nonzero = 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int big = k; float bign = nu[k];
#pragma unroll
        for (int j = k + 1; j < 3; ++j) if (nu[j] > bign) { bign = nu[j]; big = j; }
        const float big_sq = bign * bign;
        if (nonzero == 3 && big_sq < thr_helper * (float)(5 - k)) nonzero = k;
#pragma unroll
        for (int j = k + 1; j < 3; ++j) {
            if (big == j) {
#pragma unroll
                for (int i = 0; i < 5; ++i) { const float t = a[i][k]; a[i][k] = a[i][j]; a[i][j] = t; }
                { const float t = nu[k]; nu[k] = nu[j]; nu[j] = t; }
                { const float t = nd[k]; nd[k] = nd[j]; nd[j] = t; }
                const int t = perm[k]; perm[k] = perm[j]; perm[j] = t;
            }
        }
        float tail_sq = 0;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) tail_sq += a[i][k] * a[i][k];
        const float c0 = a[k][k];
        const bool tiny = tail_sq <= 1.1754943508222875e-38f;
        float beta_h = sqrtf(c0 * c0 + tail_sq);
        beta_h = c0 >= 0 ? -beta_h : beta_h;
        const float den = c0 - beta_h;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) { const float q = a[i][k] / den; a[i][k] = tiny ? 0.0f : q; }
        const float tau_h = (beta_h - c0) / beta_h;
        tau[k] = tiny ? 0.0f : tau_h;
        a[k][k] = tiny ? c0 : beta_h;
#pragma unroll
        for (int j = k + 1; j < 3; ++j) {
            float tmp = 0;
#pragma unroll
            for (int i = k + 1; i < 5; ++i) tmp += a[i][k] * a[i][j];
            tmp += a[k][j];
            a[k][j] -= tau[k] * tmp;
#pragma unroll
            for (int i = k + 1; i < 5; ++i) a[i][j] -= tau[k] * a[i][k] * tmp;
        }
#pragma unroll
        for (int j = k + 1; j < 3; ++j) {
            const bool nz = nu[j] != 0;
            float temp = fabsf(a[k][j]) / nu[j];
            temp = (1.0f + temp) * (1.0f - temp);
            temp = temp < 0 ? 0.0f : temp;
            const float r = nu[j] / nd[j];
            const float temp2 = temp * r * r;
            const bool recompute = temp2 <= downdate_thr;
            float s = 0;
#pragma unroll
            for (int i = k + 1; i < 5; ++i) s += a[i][j] * a[i][j];
            const float root = sqrtf(recompute ? s : temp);
            const float nu_new = recompute ? root : nu[j] * root;
            nd[j] = (nz && recompute) ? root : nd[j];
            nu[j] = nz ? nu_new : nu[j];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool on = k < nonzero;
        float tmp = 0;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) tmp += a[i][k] * c[i];
        tmp += c[k];
        const float ck = c[k] - tau[k] * tmp;
        c[k] = on ? ck : c[k];
#pragma unroll
        for (int i = k + 1; i < 5; ++i) { const float ci = c[i] - tau[k] * a[i][k] * tmp; c[i] = on ? ci : c[i]; }
    }
    float y[3] = {0, 0, 0};
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        float s = c[i];
#pragma unroll
        for (int j = i + 1; j < 3; ++j) { const float t = s - a[i][j] * y[j]; s = (j < nonzero) ? t : s; }
        const float q = s / a[i][i];
        y[i] = (i < nonzero) ? q : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float v = (i < nonzero) ? y[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) if (perm[i] == j) x[j] = v;
    }
}

// A x = b of a 6x6 system by unpivoted Householder QR in float (what the liorf method means by cv::solve(.., DECOMP_QR), whose own
// pivoting and summation order are not reproduced: DESIGN.md).  Column k: v = the column from the diagonal down, alpha = -sign(v0) |v|,
// v0 -= alpha, every later column and the right-hand side reflected by I - 2 v v^T / (v^T v), sums taken top to bottom; then back
// substitution.  A zero column is left alone, and an unknown whose diagonal entry is zero is 0.  M row-major.
__host__ __device__ __forceinline__ void qr6_solve_f(const float* M, const float* rhs, float* x) {
    float a[6][6], b[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        b[i] = rhs[i];
#pragma unroll
        for (int j = 0; j < 6; ++j) a[i][j] = M[i * 6 + j];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float nrm2 = 0;
#pragma unroll
        for (int i = k; i < 6; ++i) nrm2 += a[i][k] * a[i][k];
        const float nrm = sqrtf(nrm2);
        const float alpha = a[k][k] > 0 ? -nrm : nrm;
        float v[6];
#pragma unroll
        for (int i = k; i < 6; ++i) v[i] = a[i][k];
        v[k] = v[k] - alpha;
        float vv = 0;
#pragma unroll
        for (int i = k; i < 6; ++i) vv += v[i] * v[i];
        const bool skip = !(vv > 0);
#pragma unroll
        for (int j = k + 1; j < 6; ++j) {
            float dot = 0;
#pragma unroll
            for (int i = k; i < 6; ++i) dot += v[i] * a[i][j];
            const float f = 2.0f * dot / vv;
#pragma unroll
            for (int i = k; i < 6; ++i) { const float t = a[i][j] - f * v[i]; a[i][j] = skip ? a[i][j] : t; }
        }
        {
            float dot = 0;
#pragma unroll
            for (int i = k; i < 6; ++i) dot += v[i] * b[i];
            const float f = 2.0f * dot / vv;
#pragma unroll
            for (int i = k; i < 6; ++i) { const float t = b[i] - f * v[i]; b[i] = skip ? b[i] : t; }
        }
        a[k][k] = skip ? a[k][k] : alpha;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float s = b[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s -= a[i][j] * x[j];
        x[i] = a[i][i] != 0 ? s / a[i][i] : 0.0f;
    }
}

// Is the smallest eigenvalue of the symmetric 6x6 M (row-major) above t?  By Sylvester's law of inertia: M - t I is positive definite
// exactly when every pivot of its unpivoted LDL^T is positive.  In double.
__host__ __device__ __forceinline__ bool sym6_min_eig_above(const double* M, double t) {
    double m[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) m[i][j] = M[i * 6 + j] - (i == j ? t : 0.0);
    bool pd = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double piv = m[k][k];
        pd = pd && piv > 0.0;
        const double inv = pd ? 1.0 / piv : 0.0;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double l = m[i][k] * inv;
#pragma unroll
            for (int j = k + 1; j <= i; ++j) m[i][j] -= l * m[j][k];
        }
    }
    return pd;
}

}  // namespace pcr
