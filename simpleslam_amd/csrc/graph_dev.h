// graph_dev.h -- what graph_host.hip launches and graph.hip defines: the device layout of a pose graph and its three kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace pcr {
namespace graph {

// Factors in the order priors, then betweens; F of them.  Per-factor arrays are structure-of-arrays: entry k of factor e at [k * F + e].
struct Factors {
    int F;
    const int* from;          // -1: a prior
    const int* to;
    const double* z;          // [16][F] measurement (a prior: the prior pose), column-major pose entries
    const double* omega;      // [36][F] information, full symmetric, row-major entries
    const unsigned char* flags;      // [F] kFactorRobust: the robust kernel applies (between factors only); kFactorOff: switched off;
                                     //     kFactorFromFixed, kFactorToFixed: that end is a fixed pose
};
constexpr unsigned char kFactorRobust = 1, kFactorOff = 2, kFactorFromFixed = 4, kFactorToFixed = 8;

// One linearisation: per factor r (6), J_from, J_to (36 each, row-major entries) as they are; w Omega r (6), w Omega J_from, w Omega J_to with
// the factor's weight w (1; the robust kernel's w(s) on a marked factor; 0 on one switched off), which is all the solve reads of Omega;
// c = rho(s) (0 when switched off); s = r^T Omega r and the kernel's w(s) whatever the switch says (pcr_graph_between_weights).
// Fixed poses: w Omega J of an end that is a fixed pose is written as zeros (its rows and columns leave H); r, J, w Omega r, c, s and w are as
// without the flag.  What the solve reads of the unweighted J of such an end (g_p, u_e, the tree's couplings) it masks by the same two bits.
struct Lin {
    double *r, *wr, *jf, *jt, *wjf, *wjt, *c, *s, *w;
    static constexpr size_t kDoublesPerFactor = 6 + 6 + 4 * 36 + 3;
};
inline Lin lin_view(double* base, size_t F) {
    Lin l;
    l.r = base; l.wr = l.r + 6 * F; l.jf = l.wr + 6 * F; l.jt = l.jf + 36 * F; l.wjf = l.jt + 36 * F; l.wjt = l.wjf + 36 * F; l.c = l.wjt + 36 * F;
    l.s = l.c + F; l.w = l.s + F;
    return l;
}

// Incident factors of pose p: ent[row_ptr[p] .. row_ptr[p + 1]), ascending by factor, entry = factor * 2 + (1: p is the "to" end, 0: the "from" end)
struct Csr { const int* row_ptr; const int* ent; };

// Work vectors of the solve, pose-major ([p * 6 + k]); L: the preconditioner's factors [p * 21 + k]; u: per factor [e * 6 + k]
struct SolveBufs { double *x, *res, *z, *dir, *ap, *u, *L; };

// The tree preconditioner's schedule (graph_forest.h: plan_forest) and its factors, indexed by POSITION: the nodes path by path, paths by
// round, inside a path from the bottom node to the head, so that a node's heavy child is the position before it.
struct Tree {
    int R;                    // rounds
    const int* node;          // [N] position -> pose
    const int* pos_of;        // [N] pose -> position
    const int* up;            // [N] position of the parent, -1 for a root
    const int* tf;            // [N] the tree factor: factor * 2 + (1: this node is its "to" end), -1 for a root
    const int* lptr;          // [N + 1] light children of a position: lch[lptr[q] .. lptr[q + 1]), positions, ascending pose id
    const int* lch;
    const int* pbeg;          // [paths + 1] path k holds positions [pbeg[k], pbeg[k + 1])
    const int* rptr;          // [R + 1] round r holds paths [rptr[r], rptr[r + 1])
    const unsigned char* in_m;      // [F] the factor belongs to M: a prior or a tree edge
    double* G;                // [N][36] G_c = A_pc D_c^-1, row-major (p: the parent)
    double* S;                // [N][21] G_c A_cp, lower triangle: what the child takes from its parent's block
    double* y;                // [N][6] the sweeps' vector
};

// status (3 doubles, one 24-byte read per trial step): [0] chi2 of the last linearisation folded into it, [1] the solve's final
// |residual| / |g|, [2] two ints: PCG iterations, flag (0: tolerance met, 1: the cap ended it, 2: the curvature p^T A p was not positive)
constexpr int kLinBlock = 256;
constexpr int kSolveThreads = 1024;
inline int lin_blocks(int F) { return (F + kLinBlock - 1) / kLinBlock; }

// The robust kernel of the marked factors: kind = PCR_GRAPH_ROBUST_*, d = delta^2.  The kernel is chosen on the host and compiled in.
struct Robust { int kind = 0; double delta = 0.0, d = 0.0; };
// `fixed` below: the graph holds a fixed pose.  It too is chosen on the host and compiled in: a graph without one runs the instantiations that
// never look at the two bits.

// linearise every factor at `poses` into `out`, the sum of rho into status[0] (partial: lin_blocks(F) doubles)
hipError_t launch_linearize(const double* poses, const Factors& f, const Robust& rb, bool fixed, const Lin& out, double* partial, double* status,
                            hipStream_t s);
// delta (= bufs.x) <- PCG on (H + lambda I) delta = -g, one workgroup; status[1], status[2]
hipError_t launch_solve(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, double lambda, int max_it, double tol, const SolveBufs& b,
                        double* status, hipStream_t s);
// the same solve preconditioned by the spanning forest: M = lambda I + priors + tree edges, factorised once per launch (b.L by position)
hipError_t launch_solve_tree(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, const Tree& t, double lambda, int max_it, double tol,
                             const SolveBufs& b, double* status, hipStream_t s);
// z = M^-1 r by the factorisation and the sweeps of the solve of that kind (tree: the forest's; otherwise the diagonal blocks'); flag[0] = 2 when a
// block was not positive definite, else 0.  b.L, b.res (= r) and b.z are used.
hipError_t launch_precondition(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, const Tree* t, double lambda, const SolveBufs& b,
                               int* flag, hipStream_t s);
// y = (H + lambda I) x by the solve's own two passes (b.u is used)
hipError_t launch_apply(int N, const Factors& f, bool fixed, const Lin& lin, const Csr& csr, double lambda, const double* x, double* y, double* u,
                        hipStream_t s);
// out[p] = poses[p] * Exp(delta[p]); with pose_fixed (per pose, or NULL: no pose is fixed) a fixed pose's 16 doubles are copied instead
hipError_t launch_retract(int N, const double* poses, const double* delta, const unsigned char* pose_fixed, double* out, hipStream_t s);

}  // namespace graph
}  // namespace pcr
