// liorf_opt.h -- the optimiser of the liorf method as a state machine: LioScan2map::scan2MapOptimization / LMOptimization of the
// reference's test/comp/liorf_scan2map.cpp (:248-413) turned inside out, like vgicp_opt.h and ndt_opt.h.  Every decision of an iteration
// depends on 28 numbers summed over the scan -- AtA (21, upper triangle), AtB (6) and the number of rows -- which one launch of
// liorf_iterate_kernel (liorf.hip) leaves; lf_opt::ctl_step takes them in, in the prologue of the next launch, and leaves the six numbers,
// the float 4x4 and the rows' three angle matrices of the next linearisation in LiorfCtl, or `done`.  Everything is float, as in the file; the
// sums arrive in double and are rounded to float once ("liorf").
#pragma once
#include <math.h>
#include <stdint.h>

#include "pcr_internal.h"
#include "small_math.h"
#include "ndt_opt.h"      // glibc_sincosf: the C library's sinf / cosf on the device

namespace pcr {

#if defined(__HIPCC__)
#define LF_HD __host__ __device__ __forceinline__
#else
#define LF_HD inline
#endif

struct LiorfCtl {
    float six[6];            // transformTobeMapped = [roll, pitch, yaw, x, y, z]
    float T[12];             // pcl::getTransformation of them: rows 0..2 of the float 4x4, row-major (updatePointAssociateToMap)
    float G[27];             // the three 3x3 matrices (row-major) behind the angular entries of a row, for roll, pitch, yaw: lf_opt::row_matrices
    float x[6];              // the last step
    int32_t iter;            // iterCount of the next linearisation
    int32_t iters_run;       // linearisations consumed
    int32_t done, converged, degenerate, rows_last, passes, pad_;
};

// what the device-resident loop reports (host-mapped memory; `seq` is written last)
struct LiorfOut {
    float six[6];
    int32_t converged, iters_run, degenerate, rows_last, passes, pad_;
    double progress;         // seq * kProgressWindow + launches consumed so far
    double seq;
};

namespace lf_opt {

// pcl::getTransformation(x, y, z, roll, pitch, yaw) from the sines and cosines of the three angles, rows 0..2 row-major
LF_HD void transformation(const float six[6], float A, float B, float C, float D, float E, float F, float T[12]) {
    T[0] = A * C; T[1] = A * D * F - B * E; T[2] = B * F + A * D * E; T[3] = six[3];
    T[4] = B * C; T[5] = A * E + B * D * F; T[6] = B * D * E - A * F; T[7] = six[4];
    T[8] = -D; T[9] = C * F; T[10] = C * E; T[11] = six[5];
}

// The angular entries of a row (LMOptimization :306-315) are coeff . (G_a p) for three matrices that depend on the angles alone: G_a is the
// derivative of Rz(yaw) Ry(pitch) Rx(roll) with respect to angle a.  The file writes out the same matrices, with one exception: its
// line 310 has sin(pitch) in the pitch matrix's entry (1, 1), where the derivative has cos(pitch).  The method takes the derivative
// (a row is the gradient of the point's residual, and tests/test_liorf_ref.py checks all three entries by central differences).
// G: roll [0..8], pitch [9..17], yaw [18..26], each row-major.  sr / cr, sp / cp, sy / cy: sine and cosine of roll, pitch, yaw.
template <class S>
LF_HD void row_matrices(S sr, S cr, S sp, S cp, S sy, S cy, bool file_row, S G[27]) {
    const S zero = (S)0;
    S* Gr = G; S* Gp = G + 9; S* Gy = G + 18;
    Gr[0] = zero; Gr[1] = cy * sp * cr + sy * sr;   Gr[2] = sy * cr - cy * sp * sr;
    Gr[3] = zero; Gr[4] = sy * sp * cr - cy * sr;   Gr[5] = -(sy * sp * sr) - cy * cr;
    Gr[6] = zero; Gr[7] = cp * cr;                  Gr[8] = -(cp * sr);
    Gp[0] = -(cy * sp); Gp[1] = cy * cp * sr;       Gp[2] = cy * cp * cr;
    Gp[3] = -(sy * sp); Gp[4] = sy * (file_row ? sp : cp) * sr; Gp[5] = sy * cp * cr;      // [4]: the file's line 310 has sy * sp * sr (pcr_params.liorf_file_row)
    Gp[6] = -cp;        Gp[7] = -(sp * sr);         Gp[8] = -(sp * cr);
    Gy[0] = -(sy * cp); Gy[1] = -(sy * sp * sr + cy * cr); Gy[2] = cy * sr - sy * sp * cr;
    Gy[3] = cy * cp;    Gy[4] = cy * sp * sr - sy * cr;    Gy[5] = cy * sp * cr + sy * sr;
    Gy[6] = zero;       Gy[7] = zero;                      Gy[8] = zero;
}

// what the next linearisation reads: the 4x4 and the rows' matrices, of the six numbers as they stand
LF_HD void refresh(LiorfCtl* c, bool file_row) {
    const float sr = ndt_opt::glibc_sincosf(c->six[0], 0), cr = ndt_opt::glibc_sincosf(c->six[0], 1);
    const float sp = ndt_opt::glibc_sincosf(c->six[1], 0), cp = ndt_opt::glibc_sincosf(c->six[1], 1);
    const float sy = ndt_opt::glibc_sincosf(c->six[2], 0), cy = ndt_opt::glibc_sincosf(c->six[2], 1);
    transformation(c->six, cy, sy, cp, sp, cr, sr, c->T);
    row_matrices<float>(sr, cr, sp, cp, sy, cy, file_row, c->G);
}

LF_HD void ctl_init(LiorfCtl* c, const float six[6], int iters, bool file_row) {
    for (int i = 0; i < 6; ++i) { c->six[i] = six[i]; c->x[i] = 0.0f; }
    c->iter = 0; c->iters_run = 0;
    c->done = iters <= 0 ? 1 : 0;
    c->converged = 0; c->degenerate = 0; c->rows_last = 0; c->passes = 0; c->pad_ = 0;
    refresh(c, file_row);
}

// LMOptimization (:248-383) on the sums of the linearisation at c->six.  sums: AtA upper triangle row by row (21), AtB (6), rows.
LF_HD void ctl_step(LiorfCtl* c, const double sums[28], const LiorfConsts& k, LoamTrace* trace) {
    if (c->done) return;
    c->passes += 1;
    c->iters_run += 1;
    const int n = (int)sums[27];
    c->rows_last = n;
    if (n < k.min_rows) {      // (:268) `return false` with the pose untouched: every remaining iteration of the file's loop is this one again
        c->done = 1;
        return;
    }
    float A[36], b[6], x[6];
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int cc = r; cc < 6; ++cc) { A[r * 6 + cc] = A[cc * 6 + r] = (float)sums[q++]; }
#pragma unroll
    for (int r = 0; r < 6; ++r) b[r] = (float)sums[21 + r];
    qr6_solve_f(A, b, x);
    if (c->iter == 0) {        // (:332-354) only the flag is a result: the projection matP is never applied
        double Ad[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) Ad[i] = (double)A[i];
        c->degenerate = sym6_min_eig_above(Ad, k.degenerate_eig) ? 0 : 1;
    }
    if (trace) {
        LoamTrace& t = trace[c->iter];
        for (int i = 0; i < 36; ++i) t.JtJ[i] = (double)A[i];
        for (int i = 0; i < 6; ++i) { t.JtE[i] = (double)b[i]; t.x[i] = (double)x[i]; }
        t.n = n; t.cache_hits = 0; t.searches = n;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) { c->six[i] = c->six[i] + x[i]; c->x[i] = x[i]; }
    // pcl::rad2deg(float) = alpha * 57.29578f; pow(float, 2) is double; the roots are stored to float and compared in double (:370-379)
    const double r0 = (double)(x[0] * 57.29578f), r1 = (double)(x[1] * 57.29578f), r2 = (double)(x[2] * 57.29578f);
    const double t0 = (double)(x[3] * 100.0f), t1 = (double)(x[4] * 100.0f), t2 = (double)(x[5] * 100.0f);
    const float deltaR = (float)sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    const float deltaT = (float)sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    c->iter += 1;
    if ((double)deltaR < k.rot_conv_deg && (double)deltaT < k.trans_conv_cm) { c->converged = 1; c->done = 1; return; }
    if (c->iter >= k.iters) { c->done = 1; return; }
    refresh(c, k.file_row != 0);
}

}  // namespace lf_opt
}  // namespace pcr
