// graph_math.h -- SE(3) pose-graph math in f64, shared by the device kernels (graph.hip) and the host path (graph_host.hip).
//
// DESIGN.md 4.17.  Poses are 16 doubles, column-major 4x4 (T[c * 4 + r]), like every pose of the C ABI.  Tangent vectors are [omega; v],
// rotation first (GTSAM's Pose3 order, the order of vgicp_opt.h).  6x6 blocks are row-major.  Everything here is plain arithmetic plus
// sqrt and division (both correctly rounded on the host and on gfx950): sine, cosine and arc tangent are evaluated by the routines below,
// not by a math library, so that -- compiled with -ffp-contract=off -- the host and the device produce the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pcr {
namespace gm {

#define GM_HD __host__ __device__ __forceinline__

// below this squared angle the coefficient functions are evaluated by their series (theta < 0.05: the first omitted term is < 1e-18 relative)
static constexpr double kSeriesSq = 2.5e-3;

// sin and cos of x: x - k pi/2 by a three-part pi/2 (exact products while |k| < 2^20: |x| < 1.6e6, far beyond any angle met here -- larger
// arguments lose accuracy gradually and stay finite), then the Taylor polynomials on |r| <= pi/4 (r^19/19! < 1e-19).
GM_HD void sincos_d(double x, double* s, double* c) {
    const double k = floor(x * 0.63661977236758134308 + 0.5);
    double r = x - k * 1.57079632673412561417;         // pi/2, leading 33 bits
    r = r - k * 6.07710050630396597660e-11;            // next 33 bits
    r = r - k * 2.02226624879595063154e-21;            // the rest
    const double z = r * r;
    double ps = -1.0 / 121645100408832000.0;           // -1/19!
    ps = ps * z + 1.0 / 355687428096000.0;
    ps = ps * z - 1.0 / 1307674368000.0;
    ps = ps * z + 1.0 / 6227020800.0;
    ps = ps * z - 1.0 / 39916800.0;
    ps = ps * z + 1.0 / 362880.0;
    ps = ps * z - 1.0 / 5040.0;
    ps = ps * z + 1.0 / 120.0;
    ps = ps * z - 1.0 / 6.0;
    const double sr = r + r * (z * ps);
    double pc = 1.0 / 6402373705728000.0;              // 1/18!
    pc = pc * z - 1.0 / 20922789888000.0;
    pc = pc * z + 1.0 / 87178291200.0;
    pc = pc * z - 1.0 / 479001600.0;
    pc = pc * z + 1.0 / 3628800.0;
    pc = pc * z - 1.0 / 40320.0;
    pc = pc * z + 1.0 / 720.0;
    pc = pc * z - 1.0 / 24.0;
    pc = pc * z + 0.5;
    const double cr = 1.0 - z * pc;
    const long long q = (long long)k & 3;      // (values selected, then stored once each: no store through a selected pointer, which would cost scratch memory)
    const bool odd = (q & 1) != 0;
    const double sv = odd ? cr : sr, cv = odd ? sr : cr;
    const double sout = (q >= 2) ? -sv : sv;
    const double cout = (q == 1 || q == 2) ? -cv : cv;
    *s = sout;
    *c = cout;
}

// atan2(y, x) for y >= 0 (an angle in [0, pi]): the ratio of the smaller to the larger, three half-angle steps
// atan t = 2 atan(t / (1 + sqrt(1 + t^2))) down to t <= tan(pi/32), then the series to t^19.  (0, 0) gives 0.
GM_HD double atan2_pos(double y, double x) {
    const double ax = fabs(x);
    const bool swap = y > ax;
    const double hi = swap ? y : ax, lo = swap ? ax : y;
    double t = (hi > 0.0) ? lo / hi : 0.0;
    t = t / (1.0 + sqrt(1.0 + t * t));
    t = t / (1.0 + sqrt(1.0 + t * t));
    t = t / (1.0 + sqrt(1.0 + t * t));
    const double z = t * t;
    double p = -1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z - 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z - 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z - 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z - 1.0 / 3.0;
    double a = 8.0 * (t + t * (z * p));
    if (swap) a = 1.57079632679489661923 - a;          // atan(hi / lo)
    if (x < 0.0) a = 3.14159265358979323846 - a;
    return a;
}

// C = A * B, poses (the last row is 0 0 0 1 and is written as such)
GM_HD void pose_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            C[c * 4 + r] = ((A[r] * B[c * 4] + A[4 + r] * B[c * 4 + 1]) + A[8 + r] * B[c * 4 + 2]) + (c == 3 ? A[12 + r] : 0.0);
        C[c * 4 + 3] = (c == 3) ? 1.0 : 0.0;
    }
}

// B = A^-1 = [R^T, -R^T t]
GM_HD void pose_inv(const double* A, double* B) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) B[c * 4 + r] = A[r * 4 + c];
        B[12 + r] = -((A[r * 4] * A[12] + A[r * 4 + 1] * A[13]) + A[r * 4 + 2] * A[14]);
        B[r * 4 + 3] = 0.0;
    }
    B[15] = 1.0;
}

// The coefficient functions of Exp: A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3
GM_HD void exp_coeffs(double t2, double* A, double* B, double* Cc) {
    if (t2 < kSeriesSq) {
        *A = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0))));
        *B = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0))));
        *Cc = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0))));
        return;
    }
    const double t = sqrt(t2);
    double sh, ch;
    sincos_d(0.5 * t, &sh, &ch);
    const double st = 2.0 * sh * ch;
    *A = st / t;
    *B = 2.0 * sh * sh / t2;              // (no cancellation, unlike 1 - cos t)
    *Cc = (t - st) / (t2 * t);
}

// T = Exp(d), d = [omega; v]: R = I + A W + B W^2, t = (I + B W + C W^2) v
GM_HD void se3_exp(const double* d, double* T) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double t2 = (wx * wx + wy * wy) + wz * wz;
    double A, B, Cc;
    exp_coeffs(t2, &A, &B, &Cc);
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W2[i * 3 + j] = d[i] * d[j] - (i == j ? t2 : 0.0);      // W^2 = w w^T - t^2 I
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[j * 4 + i] = ((i == j ? 1.0 : 0.0) + A * W[i * 3 + j]) + B * W2[i * 3 + j];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += (((i == j ? 1.0 : 0.0) + B * W[i * 3 + j]) + Cc * W2[i * 3 + j]) * d[3 + j];
        T[12 + i] = s;
        T[i * 4 + 3] = 0.0;
    }
    T[15] = 1.0;
}

// What Log and the inverse right Jacobian share: the angle and D(theta) = (1 - (theta/2) cot(theta/2)) / theta^2, K(theta) / (2 theta) with
// K = theta / (4 sin^2(theta/2)) - cot(theta/2) / 2.  a2 = 2 D - K / (2 theta) and a4 = (D - K / (2 theta)) / theta^2 are the coefficients of
// Jr^-1(xi) = I + ad/2 + a2 ad^2 + a4 ad^4 (ad_xi satisfies x (x^2 + theta^2)^2 = 0; a2, a4 interpolate x/2 coth(x/2) on that spectrum).
struct LogCoeffs { double D, a2, a4; };
GM_HD LogCoeffs log_coeffs(double t2) {
    LogCoeffs k;
    if (t2 < kSeriesSq) {      // Bernoulli series: c1 = 1/12, c2 = -1/720, c3 = 1/30240, c4 = -1/1209600, c5 = 1/47900160
        k.D = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))));
        k.a2 = 1.0 / 12.0 + t2 * t2 * (-1.0 / 30240.0 + t2 * (-2.0 / 1209600.0 + t2 * (-3.0 / 47900160.0)));
        k.a4 = -1.0 / 720.0 + t2 * (-2.0 / 30240.0 + t2 * (-3.0 / 1209600.0 + t2 * (-4.0 / 47900160.0)));
        return k;
    }
    const double t = sqrt(t2);
    double sh, ch;
    sincos_d(0.5 * t, &sh, &ch);
    // within the contract (theta <= pi - 1e-3) sh >= 0.0248; the guard keeps every branch finite whatever comes in
    const double shs = (fabs(sh) > 1e-150) ? sh : 1e-150;
    const double cot = ch / shs;
    const double gamma = 0.5 * t * cot;
    const double kap2t = (t / (4.0 * shs * shs) - 0.5 * cot) / (2.0 * t);      // K / (2 theta)
    k.D = (1.0 - gamma) / t2;
    k.a2 = 2.0 * k.D - kap2t;
    k.a4 = (k.D - kap2t) / t2;
    return k;
}

// xi = Log(T) = [omega; v]: theta = atan2(|s|, (tr R - 1) / 2) with s = vee(R - R^T) / 2 = sin(theta) axis; omega = s theta / |s|;
// v = (I - W/2 + D W^2) t.  At theta = 0 the factor theta / |s| is 1.  Within 1e-3 of pi the axis is ill-conditioned (outside the contract):
// the numbers stay finite.
GM_HD void se3_log(const double* T, double* xi) {
    const double sx = 0.5 * (T[1 * 4 + 2] - T[2 * 4 + 1]);      // R(2,1) - R(1,2)
    const double sy = 0.5 * (T[2 * 4 + 0] - T[0 * 4 + 2]);      // R(0,2) - R(2,0)
    const double sz = 0.5 * (T[0 * 4 + 1] - T[1 * 4 + 0]);      // R(1,0) - R(0,1)
    const double sn = sqrt((sx * sx + sy * sy) + sz * sz);
    const double cs = 0.5 * (((T[0] + T[5]) + T[10]) - 1.0);
    const double theta = atan2_pos(sn, cs);
    double f;
    if (sn < 1e-4 && cs > 0.0) { const double s2 = sn * sn; f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0))); }      // asin(s) / s
    else f = (sn > 1e-300) ? theta / sn : 0.0;
    const double wx = f * sx, wy = f * sy, wz = f * sz;
    xi[0] = wx; xi[1] = wy; xi[2] = wz;
    const double t2 = (wx * wx + wy * wy) + wz * wz;
    const double D = log_coeffs(t2).D;
    const double w[3] = {wx, wy, wz};
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += (((i == j ? 1.0 : 0.0) - 0.5 * W[i * 3 + j]) + D * (w[i] * w[j] - (i == j ? t2 : 0.0))) * T[12 + j];
        xi[3 + i] = s;
    }
}

GM_HD void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}

// Jr^-1(xi) = [[Jw, 0], [Q, Jw]] (3x3 blocks, row-major): Jw = I + W/2 + D W^2,  Q = V/2 + a2 S + a4 (S W^2 + W^2 S),  S = V W + W V,
// W = omega^, V = v^ -- the blocks of I + ad/2 + a2 ad^2 + a4 ad^4 with ad = [[W, 0], [V, W]] (W^4 = -theta^2 W^2 folds a2, a4 into D on the diagonal).
GM_HD void se3_jr_inv(const double* xi, double* Jw, double* Q) {
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double t2 = (wx * wx + wy * wy) + wz * wz;
    const LogCoeffs k = log_coeffs(t2);
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    const double V[9] = {0.0, -xi[5], xi[4], xi[5], 0.0, -xi[3], -xi[4], xi[3], 0.0};
    double W2[9], VW[9], WV[9], S[9], SW2[9], W2S[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W2[i * 3 + j] = xi[i] * xi[j] - (i == j ? t2 : 0.0);
    mat3_mul(V, W, VW);
    mat3_mul(W, V, WV);
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = VW[i] + WV[i];
    mat3_mul(S, W2, SW2);
    mat3_mul(W2, S, W2S);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Jw[i] = (((i % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[i]) + k.D * W2[i];
        Q[i] = (0.5 * V[i] + k.a2 * S[i]) + k.a4 * (SW2[i] + W2S[i]);
    }
}

// One factor: E = Z^-1 Xi^-1 Xj (a prior, has_from = false: E = Z^-1 Xj), r = Log(E),
//   J_to = dr/d(delta_j) = Jr^-1(r),   J_from = dr/d(delta_i) = -Jr^-1(r) Ad((Xi^-1 Xj)^-1)   (zero for a prior)
// with Ad(T) = [[R, 0], [t^ R, R]].  Both 6x6 row-major; their upper right 3x3 blocks are zero.
GM_HD void factor_linearize(bool has_from, const double* Xi, const double* Xj, const double* Z, double* r, double* Jf, double* Jt) {
    double Zi[16], E[16], Tji[16];      // Tji = (Xi^-1 Xj)^-1
    pose_inv(Z, Zi);
    if (has_from) {
        double Xii[16], Tij[16];
        pose_inv(Xi, Xii);
        pose_mul(Xii, Xj, Tij);
        pose_mul(Zi, Tij, E);
        pose_inv(Tij, Tji);
    } else {
        pose_mul(Zi, Xj, E);
#pragma unroll
        for (int i = 0; i < 16; ++i) Tji[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    se3_log(E, r);
    double Jw[9], Q[9];
    se3_jr_inv(r, Jw, Q);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jt[i * 6 + j] = Jw[i * 3 + j];
            Jt[i * 6 + 3 + j] = 0.0;
            Jt[(3 + i) * 6 + j] = Q[i * 3 + j];
            Jt[(3 + i) * 6 + 3 + j] = Jw[i * 3 + j];
        }
    // (a prior runs the same arithmetic on an identity and selects zeros at the end: every entry of Jf has one store, which keeps the array in registers)
    double R[9], TR[9], JR[9], QR[9], JTR[9];      // R, t^ R of Tji
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = Tji[j * 4 + i];
    const double tx = Tji[12], ty = Tji[13], tz = Tji[14];
    const double Tx[9] = {0.0, -tz, ty, tz, 0.0, -tx, -ty, tx, 0.0};
    mat3_mul(Tx, R, TR);
    mat3_mul(Jw, R, JR);
    mat3_mul(Q, R, QR);
    mat3_mul(Jw, TR, JTR);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jf[i * 6 + j] = has_from ? -JR[i * 3 + j] : 0.0;
            Jf[i * 6 + 3 + j] = 0.0;
            Jf[(3 + i) * 6 + j] = has_from ? -(QR[i * 3 + j] + JTR[i * 3 + j]) : 0.0;
            Jf[(3 + i) * 6 + 3 + j] = has_from ? -JR[i * 3 + j] : 0.0;
        }
}

// Robust kernels on s = r^T Omega r (PCR_GRAPH_ROBUST_* of pcr_hip.h): rho(s) and w(s) = rho'(s), d = delta^2.  The cost of a marked factor is
// rho / 2; it enters g and H as w J^T Omega r and w J^T Omega J (the second-order term is dropped, as g2o and GTSAM drop it).
//   1 Huber          rho = s               (s <= d),  2 delta sqrt(s) - d  beyond      w = 1, delta / sqrt(s)
//   2 Geman-McClure  rho = d s / (d + s)                                               w = d^2 / (d + s)^2
//   3 Tukey          rho = d/3 (1 - (1 - s/d)^3) (s <= d),  d/3 beyond                 w = (1 - s/d)^2, 0
// Only + - * / sqrt, so host and device agree bit for bit (Cauchy's logarithm is why Cauchy is absent).  Written so that nothing overflows for any
// s >= 0: Geman-McClure through q = d / (d + s), Tukey's rho as s ((1 - q) + q^2 / 3) with q = s / d, which also spares the cancellation of
// 1 - (1 - q)^3 at small s and equals d (1/3) at s = d, the value beyond.  Huber at s = 0 divides by nothing.  Any other kind is plain least squares.
GM_HD void robust_rho_w(int kind, double s, double delta, double d, double* rho, double* w) {
    double ro = s, wo = 1.0;
    if (kind == 1) {
        if (s > d) { const double q = sqrt(s); ro = 2.0 * delta * q - d; wo = delta / q; }
    } else if (kind == 2) {
        const double q = d / (d + s);
        ro = q * s;
        wo = q * q;
    } else if (kind == 3) {
        if (s > d) { ro = d * (1.0 / 3.0); wo = 0.0; }
        else { const double q = s / d, u = 1.0 - q; ro = s * (u + q * q * (1.0 / 3.0)); wo = u * u; }
    }
    *rho = ro;
    *w = wo;
}

// Packed lower triangle: entry (i, j), j <= i, at i (i + 1) / 2 + j.
GM_HD constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// Cholesky of a symmetric positive definite 6x6 given by its lower triangle, in place: a = L with the diagonal INVERTED (the solves then
// multiply).  Returns false, leaving a unit factor, when a pivot is not positive (never for H + lambda I of a graph that passed the checks).
GM_HD bool chol6(double* a) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = a[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= a[tri(j, k)] * a[tri(j, k)];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double inv = 1.0 / sqrt(d);
        a[tri(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = a[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= a[tri(i, k)] * a[tri(j, k)];
            a[tri(i, j)] = s * inv;
        }
    }
    return ok;
}

// x = (L L^T)^-1 b with L as chol6 leaves it
GM_HD void chol6_solve(const double* l, const double* b, double* x) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= l[tri(i, k)] * y[k];
        y[i] = s * l[tri(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= l[tri(k, i)] * x[k];
        x[i] = s * l[tri(i, i)];
    }
}

#undef GM_HD
}  // namespace gm
}  // namespace pcr
