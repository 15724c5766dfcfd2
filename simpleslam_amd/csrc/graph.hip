// graph.hip -- the pose-graph back end's kernels (gfx950): linearise, solve, retract.  DESIGN.md 4.17.
//
// Backend::optimHandler (backend/src/Backend.cpp:224-347 of the reference) relinearises a GTSAM graph of one prior and one BetweenFactor per key
// frame and per loop on every key-frame event.  Here the graph lives in HBM: one launch linearises every factor (one factor per lane), one
// launch holds the whole preconditioned conjugate gradient of a Levenberg-Marquardt trial step on ONE workgroup, one launch retracts.
// Two preconditioners, a kernel each: every pose's diagonal block (graph_solve_kernel), or the spanning forest of the between factors
// solved exactly by a block Cholesky and two sweeps along a path schedule planned on the host (graph_solve_tree_kernel, graph_forest.h).
// No atomics anywhere: every sum is taken in a fixed order, so the same graph gives the same bits on every run.
#include "graph_dev.h"
#include "graph_math.h"

namespace pcr {
namespace graph {

namespace {

// sum over the wave, in lane 0 (a fixed tree: 32, 16, 8, 4, 2, 1)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- linearise: the whole grid, one factor per lane --------------------------------------------------------------------------------------
// What the solve reads of Omega are the weighted arrays written here (w Omega r, w Omega J): a robust kernel or a switch changes nothing else.
// ROBUST = PCR_GRAPH_ROBUST_*, chosen on the host.  Under NONE every weight is known up front (1, or 0 when switched off), so Omega r and
// Omega J leave row by row while s = r^T Omega r still accumulates.  A robust kind needs s before it can scale: the rows of Omega are read
// twice, first for Omega r and s, then for Omega J, and only six doubles stay live in between.
// FIXED, chosen on the host like ROBUST: the graph holds a fixed pose, and w Omega J of an end that is one leaves as zeros, as both do for a
// factor that is off.  Without it the two bits are never looked at.
template <int ROBUST, bool FIXED>
__global__ __launch_bounds__(kLinBlock) void graph_linearize_kernel(const double* __restrict__ poses, const Factors f, const Robust rb, const Lin out,
                                                                    double* __restrict__ partial) {
    __shared__ double wsum[kLinBlock / 64];
    const int F = f.F;
    const int e = blockIdx.x * kLinBlock + threadIdx.x;
    double c = 0.0;
    if (e < F) {
        const int from = f.from[e], to = f.to[e];
        const unsigned char fl = f.flags[e];
        const bool on = (fl & kFactorOff) == 0;
        const bool on_f = FIXED ? (on && (fl & kFactorFromFixed) == 0) : on, on_t = FIXED ? (on && (fl & kFactorToFixed) == 0) : on;
        double Xi[16], Xj[16], Z[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            Xj[k] = poses[(size_t)to * 16 + k];
            Xi[k] = (from >= 0) ? poses[(size_t)from * 16 + k] : 0.0;
            Z[k] = f.z[(size_t)k * F + e];
        }
        double r[6], Jf[36], Jt[36];
        gm::factor_linearize(from >= 0, Xi, Xj, Z, r, Jf, Jt);
        if constexpr (ROBUST == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double o[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) o[m] = f.omega[(size_t)(k * 6 + m) * F + e];
                double w = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) w += o[m] * r[m];
                out.r[(size_t)k * F + e] = r[k];
                out.wr[(size_t)k * F + e] = on ? w : 0.0;
                c += r[k] * w;
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    double sf = 0.0, st = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) { sf += o[m] * Jf[m * 6 + b]; st += o[m] * Jt[m * 6 + b]; }
                    out.wjf[(size_t)(k * 6 + b) * F + e] = on_f ? sf : 0.0;
                    out.wjt[(size_t)(k * 6 + b) * F + e] = on_t ? st : 0.0;
                    out.jf[(size_t)(k * 6 + b) * F + e] = Jf[k * 6 + b];
                    out.jt[(size_t)(k * 6 + b) * F + e] = Jt[k * 6 + b];
                }
            }
            out.s[e] = c;
            out.w[e] = 1.0;
            c = on ? c : 0.0;
        } else {
            double wr[6], s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double w = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) w += f.omega[(size_t)(k * 6 + m) * F + e] * r[m];
                out.r[(size_t)k * F + e] = r[k];
                wr[k] = w;
                s += r[k] * w;
            }
            double rho, wk;
            gm::robust_rho_w((fl & kFactorRobust) ? ROBUST : 0, s, rb.delta, rb.d, &rho, &wk);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double o[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) o[m] = f.omega[(size_t)(k * 6 + m) * F + e];
                out.wr[(size_t)k * F + e] = on ? wk * wr[k] : 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    double sf = 0.0, st = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) { sf += o[m] * Jf[m * 6 + b]; st += o[m] * Jt[m * 6 + b]; }
                    out.wjf[(size_t)(k * 6 + b) * F + e] = on_f ? wk * sf : 0.0;
                    out.wjt[(size_t)(k * 6 + b) * F + e] = on_t ? wk * st : 0.0;
                    out.jf[(size_t)(k * 6 + b) * F + e] = Jf[k * 6 + b];
                    out.jt[(size_t)(k * 6 + b) * F + e] = Jt[k * 6 + b];
                }
            }
            out.s[e] = s;
            out.w[e] = wk;
            c = on ? rho : 0.0;
        }
        out.c[e] = c;
    }
    // chi2: lanes past the end add 0; the wave's tree, then the block's four waves in order
    const double ws = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one wave folds the blocks' partial sums: lane l takes blocks l, l + 64, ... in that order, then the tree
__global__ __launch_bounds__(64) void graph_chi2_fold_kernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ status) {
    double s = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 64) s += partial[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) status[0] = s;
}

// ---- the two passes of y = (H + lambda I) x, shared by the solve and by pcr_graph_apply --------------------------------------------------
// Fixed poses (FIXED: the graph holds one).  The linearisation wrote zeros for Omega J of a fixed end, which alone makes the pose's row of H
// vanish (pose_product), its diagonal block lambda I and the tree's coupling A_qp zero when the PARENT is fixed.  Three terms read the
// unweighted J of an end and are masked by the factor's two bits: u_e (below: x of a fixed end counts as 0, its column of H), g_p (the set-up
// loops leave a fixed pose's row out altogether: J_p^T w Omega r is not taken, and its block J_p^T (w Omega J_p) would be a sum of zeros) and
// A_qp when the CHILD is fixed (tree_factorize).  With these g_p = 0, res_p = z_p = dir_p = 0 from the start, and the
// conjugate gradient keeps x_p at exactly 0 under both preconditioners.
__device__ __forceinline__ bool end_is_fixed(const Factors& f, int ent) {
    return (f.flags[ent >> 1] & ((ent & 1) ? kFactorToFixed : kFactorFromFixed)) != 0;
}

// pass 1, over the factors: u_e = J_from x_from + J_to x_to
template <bool FIXED>
__device__ __forceinline__ void edge_pass(const Factors& f, const Lin& lin, const double* __restrict__ x, double* __restrict__ u, int tid, int nthreads) {
    const int F = f.F;
    for (int e = tid; e < F; e += nthreads) {
        const int from = f.from[e], to = f.to[e];
        double xt[6], xf[6], acc[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { xt[k] = x[(size_t)to * 6 + k]; xf[k] = (from >= 0) ? x[(size_t)from * 6 + k] : 0.0; }
        if (FIXED) {
            const unsigned char fl = f.flags[e];
#pragma unroll
            for (int k = 0; k < 6; ++k) { if (fl & kFactorToFixed) xt[k] = 0.0; if (fl & kFactorFromFixed) xf[k] = 0.0; }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) s += lin.jt[(size_t)(k * 6 + m) * F + e] * xt[m];
            if (from >= 0) {
#pragma unroll
                for (int m = 0; m < 6; ++m) s += lin.jf[(size_t)(k * 6 + m) * F + e] * xf[m];
            }
            acc[k] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) u[(size_t)e * 6 + k] = acc[k];
    }
}

// pass 2, one pose: y_p = lambda x_p + sum over p's incident factors, in CSR order, of (Omega J_p)^T u_e
__device__ __forceinline__ void pose_product(int p, const Factors& f, const Lin& lin, const Csr& csr, double lambda, const double* xp,
                                             const double* __restrict__ u, double* y) {
    const int F = f.F;
#pragma unroll
    for (int k = 0; k < 6; ++k) y[k] = lambda * xp[k];
    const int lo = csr.row_ptr[p], hi = csr.row_ptr[p + 1];
    for (int i = lo; i < hi; ++i) {
        const int ent = csr.ent[i];
        const int e = ent >> 1;
        const double* __restrict__ wj = (ent & 1) ? lin.wjt : lin.wjf;
        double ue[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) ue[k] = u[(size_t)e * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int m = 0; m < 6; ++m) y[m] += wj[(size_t)(k * 6 + m) * F + e] * ue[k];
        }
    }
}

// block-wide sums of NV values, the same bits in every thread: the wave's tree, then the 16 waves in order.  `lds` holds NV * 16 doubles and is
// not written again before another barrier has passed (the call sites alternate between two arrays).
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* lds) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0) lds[i * 16 + (threadIdx.x >> 6)] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kSolveThreads / 64; ++w) s += lds[i * 16 + w];
        v[i] = s;
    }
}

// one pose's gradient g_p and its diagonal block of the preconditioner (lower triangle), over p's incident factors in CSR order:
// lambda I + sum J^T Omega J -- over every factor for the block-diagonal preconditioner, over the priors and the tree edges (in_m) for the
// tree's.  g takes every factor either way.
template <bool TREE, bool FIXED>
__device__ __forceinline__ void pose_blocks(int p, const Factors& f, const Lin& lin, const Csr& csr, const unsigned char* __restrict__ in_m,
                                            double lambda, double* g, double* D) {
    const int F = f.F;
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) D[gm::tri(i, j)] = (i == j) ? lambda : 0.0;
    // p is a fixed pose (every entry of its row says so): its row is left out, g_p = 0 and the block lambda I
    const int lo = csr.row_ptr[p], row_end = csr.row_ptr[p + 1];
    const int hi = (FIXED && lo < row_end && end_is_fixed(f, csr.ent[lo])) ? lo : row_end;
    for (int i = lo; i < hi; ++i) {
        const int ent = csr.ent[i];
        const int e = ent >> 1;
        const double* __restrict__ J = (ent & 1) ? lin.jt : lin.jf;
        const double* __restrict__ WJ = (ent & 1) ? lin.wjt : lin.wjf;
        const bool in_block = TREE ? (in_m[e] != 0) : true;
#pragma unroll
        for (int k = 0; k < 6; ++k) {      // row k of J and of Omega J: a rank-one update of the block, one term of g
            double jr[6], wr6[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) { jr[m] = J[(size_t)(k * 6 + m) * F + e]; wr6[m] = WJ[(size_t)(k * 6 + m) * F + e]; }
            const double wrk = lin.wr[(size_t)k * F + e];
#pragma unroll
            for (int m = 0; m < 6; ++m) g[m] += jr[m] * wrk;
            if (in_block) {
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) D[gm::tri(r, c)] += jr[r] * wr6[c];
            }
        }
    }
}

// ---- the tree preconditioner: M = lambda I + the priors + the forest's between factors, block Cholesky from the leaves to the roots -------
// The schedule is graph_forest.h's: one lane walks one path, the paths of a round run on different lanes, a barrier separates the rounds.
// A node gathers from its heavy child (the position before it, carried in registers) and then from its light children in ascending id,
// whose results an earlier round finished: nothing is scattered, the order of every sum is fixed.
//
// On entry L[q] holds position q's diagonal block of M (a barrier has passed since it was written).  On return L[q] is the Cholesky factor
// of D_q = A_qq - sum over children G_c A_cq, t.G[q] = A_pq D_q^-1 for the parent p, and a barrier has passed.  false: some D_q of this
// lane's was not positive definite.
template <bool FIXED>
__device__ __forceinline__ bool tree_factorize(const Factors& f, const Lin& lin, const Tree& t, double* __restrict__ L, int tid) {
    const int F = f.F;
    bool ok = true;
    for (int r = 0; r < t.R; ++r) {
        for (int path = t.rptr[r] + tid; path < t.rptr[r + 1]; path += kSolveThreads) {
            const int q0 = t.pbeg[path], q1 = t.pbeg[path + 1];
            double Sp[21];      // G_c A_cq of the node below
#pragma unroll
            for (int k = 0; k < 21; ++k) Sp[k] = 0.0;
            for (int q = q0; q < q1; ++q) {
                double D[21];
#pragma unroll
                for (int k = 0; k < 21; ++k) D[k] = L[(size_t)q * 21 + k] - Sp[k];
                for (int i = t.lptr[q]; i < t.lptr[q + 1]; ++i) {
                    const int c = t.lch[i];
#pragma unroll
                    for (int k = 0; k < 21; ++k) D[k] -= t.S[(size_t)c * 21 + k];
                }
                ok = gm::chol6(D) && ok;
#pragma unroll
                for (int k = 0; k < 21; ++k) L[(size_t)q * 21 + k] = D[k];
                const int ent = t.tf[q];
                if (ent < 0) continue;      // a root
                const int e = ent >> 1;
                const double* __restrict__ J = (ent & 1) ? lin.jt : lin.jf;        // this node's end
                const double* __restrict__ WJ = (ent & 1) ? lin.wjf : lin.wjt;     // Omega J of the parent's end
                if (FIXED && end_is_fixed(f, ent)) {      // this node is a fixed pose: no coupling to its parent, A_qp = 0
#pragma unroll
                    for (int k = 0; k < 36; ++k) t.G[(size_t)q * 36 + k] = 0.0;
#pragma unroll
                    for (int k = 0; k < 21; ++k) Sp[k] = 0.0;
                    if (q == q1 - 1) {
#pragma unroll
                        for (int k = 0; k < 21; ++k) t.S[(size_t)q * 21 + k] = 0.0;
                    }
                    continue;
                }
                double A[36];      // A_qp = J_q^T Omega J_p, rows in this node's space
#pragma unroll
                for (int k = 0; k < 36; ++k) A[k] = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) {
                    double jr[6], wr6[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) { jr[k] = J[(size_t)(m * 6 + k) * F + e]; wr6[k] = WJ[(size_t)(m * 6 + k) * F + e]; }
#pragma unroll
                    for (int k = 0; k < 6; ++k)
#pragma unroll
                        for (int j = 0; j < 6; ++j) A[k * 6 + j] += jr[k] * wr6[j];
                }
                double G[36];      // row j: D_q^-1 (column j of A_qp)
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    double a[6], s[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) a[k] = A[k * 6 + j];
                    gm::chol6_solve(D, a, s);
#pragma unroll
                    for (int k = 0; k < 6; ++k) { G[j * 6 + k] = s[k]; t.G[(size_t)q * 36 + j * 6 + k] = s[k]; }
                }
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; ++k) s += G[i * 6 + k] * A[k * 6 + j];
                        Sp[gm::tri(i, j)] = s;
                    }
                if (q == q1 - 1) {      // a head: its parent reads it from memory in a later round
#pragma unroll
                    for (int k = 0; k < 21; ++k) t.S[(size_t)q * 21 + k] = Sp[k];
                }
            }
        }
        __syncthreads();
    }
    return ok;
}

// z = M^-1 r: r by pose (a barrier has passed since it was written), z in t.y by POSITION; a barrier has passed on return.
// Forward y_q = r_q - sum over children G_c y_c, rounds ascending; then D_q^-1 y_q for all positions at once, so that only the 6x6 product
// is on the serial chain of the way down, z_q = D_q^-1 y_q - G_q^T z_parent, rounds descending.
__device__ __forceinline__ void tree_solve(int N, const Tree& t, const double* __restrict__ L, const double* __restrict__ r, int tid) {
    for (int q = tid; q < N; q += kSolveThreads) {
        const int p = t.node[q];
#pragma unroll
        for (int k = 0; k < 6; ++k) t.y[(size_t)q * 6 + k] = r[(size_t)p * 6 + k];
    }
    __syncthreads();
    for (int rd = 0; rd < t.R; ++rd) {
        for (int path = t.rptr[rd] + tid; path < t.rptr[rd + 1]; path += kSolveThreads) {
            const int q0 = t.pbeg[path], q1 = t.pbeg[path + 1];
            double yp[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) yp[k] = 0.0;
            for (int q = q0; q < q1; ++q) {
                double y[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) y[k] = t.y[(size_t)q * 6 + k];
                if (q > q0) {
                    const double* __restrict__ G = t.G + (size_t)(q - 1) * 36;
#pragma unroll
                    for (int j = 0; j < 6; ++j)
#pragma unroll
                        for (int k = 0; k < 6; ++k) y[j] -= G[j * 6 + k] * yp[k];
                }
                for (int i = t.lptr[q]; i < t.lptr[q + 1]; ++i) {
                    const int c = t.lch[i];
                    const double* __restrict__ G = t.G + (size_t)c * 36;
                    double yc[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) yc[k] = t.y[(size_t)c * 6 + k];
#pragma unroll
                    for (int j = 0; j < 6; ++j)
#pragma unroll
                        for (int k = 0; k < 6; ++k) y[j] -= G[j * 6 + k] * yc[k];
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) { t.y[(size_t)q * 6 + k] = y[k]; yp[k] = y[k]; }
            }
        }
        __syncthreads();
    }
    for (int q = tid; q < N; q += kSolveThreads) {
        double Lq[21], y[6], w[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) Lq[k] = L[(size_t)q * 21 + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) y[k] = t.y[(size_t)q * 6 + k];
        gm::chol6_solve(Lq, y, w);
#pragma unroll
        for (int k = 0; k < 6; ++k) t.y[(size_t)q * 6 + k] = w[k];
    }
    __syncthreads();
    for (int rd = t.R - 1; rd >= 0; --rd) {
        for (int path = t.rptr[rd] + tid; path < t.rptr[rd + 1]; path += kSolveThreads) {
            const int q0 = t.pbeg[path], q1 = t.pbeg[path + 1];
            const int up = t.up[q1 - 1];
            bool has = up >= 0;
            double zp[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) zp[k] = has ? t.y[(size_t)up * 6 + k] : 0.0;
            for (int q = q1 - 1; q >= q0; --q) {
                double z[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) z[k] = t.y[(size_t)q * 6 + k];
                if (has) {
                    const double* __restrict__ G = t.G + (size_t)q * 36;
#pragma unroll
                    for (int j = 0; j < 6; ++j)
#pragma unroll
                        for (int k = 0; k < 6; ++k) z[k] -= G[j * 6 + k] * zp[j];
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) { t.y[(size_t)q * 6 + k] = z[k]; zp[k] = z[k]; }
                has = true;
            }
        }
        __syncthreads();
    }
}

// ---- solve: the whole PCG of one trial step on one workgroup ------------------------------------------------------------------------------
// (H + lambda I) x = -g with H = sum J^T Omega J, g = sum J^T Omega r; preconditioner: the inverse of every pose's 6x6 diagonal block.
// Threads stride over the poses and over the factors.  Writes are made visible to the workgroup by the barriers: one workgroup is one CU.
template <bool FIXED>
__global__ __launch_bounds__(kSolveThreads) void graph_solve_kernel(const int N, const Factors f, const Lin lin, const Csr csr, const double lambda,
                                                                    const int max_it, const double tol, const SolveBufs b, double* __restrict__ status) {
    __shared__ double red_a[2 * 16], red_b[2 * 16];
    const int tid = threadIdx.x;
    const int F = f.F;

    // set-up: g_p, the diagonal block, its Cholesky factor; x = 0, res = -g, z = M^-1 res, dir = z
    double acc[2] = {0.0, 0.0};      // |g|^2, res . z
    for (int p = tid; p < N; p += kSolveThreads) {
        double g[6], D[21];      // (pose_blocks<false, FIXED> below, kept inline: this kernel's code and registers are as they were measured)
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) D[gm::tri(i, j)] = (i == j) ? lambda : 0.0;
        const int lo = csr.row_ptr[p], row_end = csr.row_ptr[p + 1];
        const int hi = (FIXED && lo < row_end && end_is_fixed(f, csr.ent[lo])) ? lo : row_end;      // a fixed pose's row is left out: g_p = 0, the block lambda I
        for (int i = lo; i < hi; ++i) {
            const int ent = csr.ent[i];
            const int e = ent >> 1;
            const double* __restrict__ J = (ent & 1) ? lin.jt : lin.jf;
            const double* __restrict__ WJ = (ent & 1) ? lin.wjt : lin.wjf;
#pragma unroll
            for (int k = 0; k < 6; ++k) {      // row k of J and of Omega J: a rank-one update of the block, one term of g
                double jr[6], wr6[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) { jr[m] = J[(size_t)(k * 6 + m) * F + e]; wr6[m] = WJ[(size_t)(k * 6 + m) * F + e]; }
                const double wrk = lin.wr[(size_t)k * F + e];
#pragma unroll
                for (int m = 0; m < 6; ++m) g[m] += jr[m] * wrk;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) D[gm::tri(r, c)] += jr[r] * wr6[c];
            }
        }
        gm::chol6(D);
        double res[6], z[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) res[k] = -g[k];
        gm::chol6_solve(D, res, z);
#pragma unroll
        for (int k = 0; k < 21; ++k) b.L[(size_t)p * 21 + k] = D[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            b.x[(size_t)p * 6 + k] = 0.0;
            b.res[(size_t)p * 6 + k] = res[k];
            b.dir[(size_t)p * 6 + k] = z[k];
            acc[0] += g[k] * g[k];
            acc[1] += res[k] * z[k];
        }
    }
    block_sum(acc, red_b);
    const double gnorm = sqrt(acc[0]);
    double rz = acc[1];
    double relres = (gnorm > 0.0) ? 1.0 : 0.0;
    int it = 0, flag = (gnorm > 0.0) ? 1 : 0;      // (1 until the tolerance is met: a loop that runs out was ended by the cap)
    if (gnorm > 0.0 && relres <= tol) flag = 0;

    while (flag == 1 && it < max_it) {
        // (a barrier stands between the writes of dir and this pass: the set-up's block_sum on entry, the loop's own afterwards)
        edge_pass<FIXED>(f, lin, b.dir, b.u, tid, kSolveThreads);
        __syncthreads();
        double pap[1] = {0.0};
        for (int p = tid; p < N; p += kSolveThreads) {
            double d[6], y[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = b.dir[(size_t)p * 6 + k];
            pose_product(p, f, lin, csr, lambda, d, b.u, y);
#pragma unroll
            for (int k = 0; k < 6; ++k) { b.ap[(size_t)p * 6 + k] = y[k]; pap[0] += d[k] * y[k]; }
        }
        block_sum(pap, red_a);
        if (!(pap[0] > 0.0)) { flag = 2; break; }
        const double alpha = rz / pap[0];
        double nn[2] = {0.0, 0.0};      // res . z, |res|^2 after the update
        for (int p = tid; p < N; p += kSolveThreads) {
            double res[6], z[6], L[21];
#pragma unroll
            for (int k = 0; k < 21; ++k) L[k] = b.L[(size_t)p * 21 + k];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                b.x[(size_t)p * 6 + k] += alpha * b.dir[(size_t)p * 6 + k];
                res[k] = b.res[(size_t)p * 6 + k] - alpha * b.ap[(size_t)p * 6 + k];
                b.res[(size_t)p * 6 + k] = res[k];
            }
            gm::chol6_solve(L, res, z);
#pragma unroll
            for (int k = 0; k < 6; ++k) { b.z[(size_t)p * 6 + k] = z[k]; nn[0] += res[k] * z[k]; nn[1] += res[k] * res[k]; }
        }
        block_sum(nn, red_b);
        ++it;
        relres = sqrt(nn[1]) / gnorm;
        if (!(relres > tol)) { flag = 0; break; }      // (a residual that is not a number ends the loop too: the host sees it in relres)
        const double beta = nn[0] / rz;
        rz = nn[0];
        for (int p = tid; p < N; p += kSolveThreads) {      // every thread updates the poses it owns: nobody else reads dir before the next barrier
#pragma unroll
            for (int k = 0; k < 6; ++k) b.dir[(size_t)p * 6 + k] = b.z[(size_t)p * 6 + k] + beta * b.dir[(size_t)p * 6 + k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        status[1] = relres;
        int* w = reinterpret_cast<int*>(status + 2);
        w[0] = it;
        w[1] = flag;
    }
}

// The same PCG with the tree preconditioner.  M is factorised once per launch (lambda and the linearisation change per trial step); a block
// that is not positive definite ends the launch with flag 2 and x = 0, as a curvature that is not positive does.  b.L is indexed by position.
template <bool FIXED>
__global__ __launch_bounds__(kSolveThreads) void graph_solve_tree_kernel(const int N, const Factors f, const Lin lin, const Csr csr, const Tree t,
                                                                         const double lambda, const int max_it, const double tol, const SolveBufs b,
                                                                         double* __restrict__ status) {
    __shared__ double red_a[2 * 16], red_b[2 * 16];
    const int tid = threadIdx.x;

    // set-up: g_p and the pose's block of M; x = 0, res = -g
    double gg[1] = {0.0};
    for (int q = tid; q < N; q += kSolveThreads) {
        const int p = t.node[q];
        double g[6], D[21];
        pose_blocks<true, FIXED>(p, f, lin, csr, t.in_m, lambda, g, D);
#pragma unroll
        for (int k = 0; k < 21; ++k) b.L[(size_t)q * 21 + k] = D[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            b.x[(size_t)p * 6 + k] = 0.0;
            b.res[(size_t)p * 6 + k] = -g[k];
            gg[0] += g[k] * g[k];
        }
    }
    block_sum(gg, red_b);      // (its barrier stands between the blocks' writes and the factorisation)
    const bool ok = tree_factorize<FIXED>(f, lin, t, b.L, tid);
    const int bad = __syncthreads_or(ok ? 0 : 1);
    const double gnorm = sqrt(gg[0]);
    double relres = (gnorm > 0.0) ? 1.0 : 0.0;
    int it = 0, flag = (gnorm > 0.0) ? 1 : 0;
    if (gnorm > 0.0 && relres <= tol) flag = 0;
    if (bad) flag = 2;
    double rz = 0.0;
    if (flag == 1) {      // z = M^-1 res, dir = z
        tree_solve(N, t, b.L, b.res, tid);
        double acc[1] = {0.0};
        for (int p = tid; p < N; p += kSolveThreads) {
            const int q = t.pos_of[p];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double z = t.y[(size_t)q * 6 + k];
                b.dir[(size_t)p * 6 + k] = z;
                acc[0] += b.res[(size_t)p * 6 + k] * z;
            }
        }
        block_sum(acc, red_a);
        rz = acc[0];
    }

    while (flag == 1 && it < max_it) {
        edge_pass<FIXED>(f, lin, b.dir, b.u, tid, kSolveThreads);
        __syncthreads();
        double pap[1] = {0.0};
        for (int p = tid; p < N; p += kSolveThreads) {
            double d[6], y[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = b.dir[(size_t)p * 6 + k];
            pose_product(p, f, lin, csr, lambda, d, b.u, y);
#pragma unroll
            for (int k = 0; k < 6; ++k) { b.ap[(size_t)p * 6 + k] = y[k]; pap[0] += d[k] * y[k]; }
        }
        block_sum(pap, red_b);
        if (!(pap[0] > 0.0)) { flag = 2; break; }
        const double alpha = rz / pap[0];
        double rr[1] = {0.0};      // |res|^2 after the update
        for (int p = tid; p < N; p += kSolveThreads) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                b.x[(size_t)p * 6 + k] += alpha * b.dir[(size_t)p * 6 + k];
                const double res = b.res[(size_t)p * 6 + k] - alpha * b.ap[(size_t)p * 6 + k];
                b.res[(size_t)p * 6 + k] = res;
                rr[0] += res * res;
            }
        }
        block_sum(rr, red_a);
        ++it;
        relres = sqrt(rr[0]) / gnorm;
        if (!(relres > tol)) { flag = 0; break; }
        tree_solve(N, t, b.L, b.res, tid);
        double nz[1] = {0.0};      // res . z
        for (int p = tid; p < N; p += kSolveThreads) {
            const int q = t.pos_of[p];
#pragma unroll
            for (int k = 0; k < 6; ++k) nz[0] += b.res[(size_t)p * 6 + k] * t.y[(size_t)q * 6 + k];
        }
        block_sum(nz, red_b);
        const double beta = nz[0] / rz;
        rz = nz[0];
        for (int p = tid; p < N; p += kSolveThreads) {
            const int q = t.pos_of[p];
#pragma unroll
            for (int k = 0; k < 6; ++k) b.dir[(size_t)p * 6 + k] = t.y[(size_t)q * 6 + k] + beta * b.dir[(size_t)p * 6 + k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        status[1] = relres;
        int* w = reinterpret_cast<int*>(status + 2);
        w[0] = it;
        w[1] = flag;
    }
}

// pcr_graph_precondition: z = M^-1 r by the factorisation and the sweeps of the solve of that kind; r in b.res, z into b.z, both by pose
template <bool TREE, bool FIXED>
__global__ __launch_bounds__(kSolveThreads) void graph_precondition_kernel(const int N, const Factors f, const Lin lin, const Csr csr, const Tree t,
                                                                           const double lambda, const SolveBufs b, int* __restrict__ flag) {
    const int tid = threadIdx.x;
    bool ok = true;
    if (TREE) {
        for (int q = tid; q < N; q += kSolveThreads) {
            double g[6], D[21];
            pose_blocks<true, FIXED>(t.node[q], f, lin, csr, t.in_m, lambda, g, D);
#pragma unroll
            for (int k = 0; k < 21; ++k) b.L[(size_t)q * 21 + k] = D[k];
        }
        __syncthreads();
        ok = tree_factorize<FIXED>(f, lin, t, b.L, tid);
        tree_solve(N, t, b.L, b.res, tid);
        for (int p = tid; p < N; p += kSolveThreads) {
            const int q = t.pos_of[p];
#pragma unroll
            for (int k = 0; k < 6; ++k) b.z[(size_t)p * 6 + k] = t.y[(size_t)q * 6 + k];
        }
    } else {
        for (int p = tid; p < N; p += kSolveThreads) {
            double g[6], D[21], res[6], z[6];
            pose_blocks<false, FIXED>(p, f, lin, csr, nullptr, lambda, g, D);
            ok = gm::chol6(D) && ok;
#pragma unroll
            for (int k = 0; k < 6; ++k) res[k] = b.res[(size_t)p * 6 + k];
            gm::chol6_solve(D, res, z);
#pragma unroll
            for (int k = 0; k < 6; ++k) b.z[(size_t)p * 6 + k] = z[k];
        }
    }
    const int bad = __syncthreads_or(ok ? 0 : 1);
    if (tid == 0) flag[0] = bad ? 2 : 0;
}

template <bool FIXED>
__global__ __launch_bounds__(kSolveThreads) void graph_apply_kernel(const int N, const Factors f, const Lin lin, const Csr csr, const double lambda,
                                                                    const double* __restrict__ x, double* __restrict__ y, double* __restrict__ u) {
    edge_pass<FIXED>(f, lin, x, u, threadIdx.x, kSolveThreads);
    __syncthreads();
    for (int p = threadIdx.x; p < N; p += kSolveThreads) {
        double xp[6], yp[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) xp[k] = x[(size_t)p * 6 + k];
        pose_product(p, f, lin, csr, lambda, xp, u, yp);
#pragma unroll
        for (int k = 0; k < 6; ++k) y[(size_t)p * 6 + k] = yp[k];
    }
}

// ---- retract: X_trial = X Exp(delta) ----------------------------------------------------------------------------------------------------
// A fixed pose's 16 doubles are COPIED (FIXED; pose_fixed per pose): its delta is 0, but nothing here rests on X Exp(0) returning X's bits.
template <bool FIXED>
__global__ __launch_bounds__(256) void graph_retract_kernel(const int N, const double* __restrict__ poses, const double* __restrict__ delta,
                                                            const unsigned char* __restrict__ pose_fixed, double* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    double X[16], d[6], E[16], Y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) X[k] = poses[(size_t)p * 16 + k];
    if (FIXED && pose_fixed[p]) {
#pragma unroll
        for (int k = 0; k < 16; ++k) out[(size_t)p * 16 + k] = X[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = delta[(size_t)p * 6 + k];
    gm::se3_exp(d, E);
    gm::pose_mul(X, E, Y);
#pragma unroll
    for (int k = 0; k < 16; ++k) out[(size_t)p * 16 + k] = Y[k];
}

}  // namespace

hipError_t launch_linearize(const double* poses, const Factors& f, const Robust& rb, bool fixed, const Lin& out, double* partial, double* status,
                            hipStream_t s) {
    const int nb = lin_blocks(f.F);
    if (nb > 0) {
#define PCR_GRAPH_LIN(K) \
    if (fixed) hipLaunchKernelGGL((graph_linearize_kernel<K, true>), dim3(nb), dim3(kLinBlock), 0, s, poses, f, rb, out, partial); \
    else hipLaunchKernelGGL((graph_linearize_kernel<K, false>), dim3(nb), dim3(kLinBlock), 0, s, poses, f, rb, out, partial)
        switch (rb.kind) {
            case 0: PCR_GRAPH_LIN(0); break;
            case 1: PCR_GRAPH_LIN(1); break;
            case 2: PCR_GRAPH_LIN(2); break;
            case 3: PCR_GRAPH_LIN(3); break;
            default: return hipErrorInvalidValue;      // (pcr_graph_set_robust_kernel refuses every other kind)
        }
#undef PCR_GRAPH_LIN
    }
    hipLaunchKernelGGL(graph_chi2_fold_kernel, dim3(1), dim3(64), 0, s, partial, nb, status);
    return hipGetLastError();
}

hipError_t launch_solve(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, double lambda, int max_it, double tol, const SolveBufs& b,
                        double* status, hipStream_t s) {
    if (fixed) hipLaunchKernelGGL(graph_solve_kernel<true>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, lambda, max_it, tol, b, status);
    else hipLaunchKernelGGL(graph_solve_kernel<false>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, lambda, max_it, tol, b, status);
    return hipGetLastError();
}

hipError_t launch_solve_tree(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, const Tree& t, double lambda, int max_it, double tol,
                             const SolveBufs& b, double* status, hipStream_t s) {
    if (fixed) hipLaunchKernelGGL(graph_solve_tree_kernel<true>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, t, lambda, max_it, tol, b, status);
    else hipLaunchKernelGGL(graph_solve_tree_kernel<false>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, t, lambda, max_it, tol, b, status);
    return hipGetLastError();
}

hipError_t launch_precondition(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, const Tree* t, double lambda, const SolveBufs& b,
                               int* flag, hipStream_t s) {
    const Tree tr = t ? *t : Tree{};
    if (t && fixed) hipLaunchKernelGGL((graph_precondition_kernel<true, true>), dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, tr, lambda, b, flag);
    else if (t) hipLaunchKernelGGL((graph_precondition_kernel<true, false>), dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, tr, lambda, b, flag);
    else if (fixed) hipLaunchKernelGGL((graph_precondition_kernel<false, true>), dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, tr, lambda, b, flag);
    else hipLaunchKernelGGL((graph_precondition_kernel<false, false>), dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, tr, lambda, b, flag);
    return hipGetLastError();
}

hipError_t launch_apply(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, double lambda, const double* x, double* y, double* u,
                        hipStream_t s) {
    if (fixed) hipLaunchKernelGGL(graph_apply_kernel<true>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, lambda, x, y, u);
    else hipLaunchKernelGGL(graph_apply_kernel<false>, dim3(1), dim3(kSolveThreads), 0, s, N, f, lin, csr, lambda, x, y, u);
    return hipGetLastError();
}

hipError_t launch_retract(int N, const double* poses, const double* delta, const unsigned char* pose_fixed, double* out, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (pose_fixed) hipLaunchKernelGGL(graph_retract_kernel<true>, dim3((N + 255) / 256), dim3(256), 0, s, N, poses, delta, pose_fixed, out);
    else hipLaunchKernelGGL(graph_retract_kernel<false>, dim3((N + 255) / 256), dim3(256), 0, s, N, poses, delta, pose_fixed, out);
    return hipGetLastError();
}

}  // namespace graph
}  // namespace pcr
