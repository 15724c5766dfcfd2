"""Fixed poses ("Fixed poses") restated in numpy on top of graph_ref and graph_robust_ref: the same residuals, Jacobians,
robust weights, lm_decisions controller and stall rule; the dense normal equations are reduced to the free poses' rows and columns and
solved densely, and a fixed pose is never touched.

A pose that carries the fixed flag is a constant of the problem.  chi2 stays the sum over every factor that is switched on (a factor between
two fixed poses is a constant term and counts).  With no pose fixed, optimize() performs graph_ref.Graph.optimize's operations one for one."""
import numpy as np

import graph_ref as gr
import graph_robust_ref as rr


class FixedGraph(rr.RobustGraph):
    """graph_robust_ref.RobustGraph plus a fixed flag per pose (self.fixed: a set of ids)."""

    def __init__(self):
        super().__init__()
        self.fixed = set()

    @classmethod
    def of(cls, g, fixed=()):
        """a FixedGraph holding graph_ref.Graph or RobustGraph g (copied), the poses `fixed` fixed"""
        f = cls()
        f.poses = [p.copy() for p in g.poses]
        f.priors, f.betweens = list(g.priors), list(g.betweens)
        f.kind, f.delta = getattr(g, "kind", rr.NONE), getattr(g, "delta", 0.0)
        f.robust = list(getattr(g, "robust", [False] * len(g.betweens)))
        f.enabled = list(getattr(g, "enabled", [True] * len(g.betweens)))
        f.fixed = set(int(k) for k in fixed)
        assert all(0 <= k < len(f.poses) for k in f.fixed)
        return f

    def copy(self):
        return FixedGraph.of(self, self.fixed)

    def free_index(self, n=None):
        """the rows of the 6N system that belong to free poses, ascending"""
        n = len(self.poses) if n is None else n
        return np.array([6 * p + k for p in range(n) if p not in self.fixed for k in range(6)], dtype=np.int64)

    def reduced_equations(self, poses=None):
        """-> H_ff, g_f, chi2, free: the full problem's normal equations with the fixed poses' rows and columns removed"""
        H, g, chi2 = self.normal_equations(poses)
        free = self.free_index()
        return H[np.ix_(free, free)], g[free], chi2, free

    def optimize(self, **params):
        """graph_ref.Graph.optimize over the free poses: -> dict(iterations, accepted, chi2_initial, chi2_final, lambda_, converged);
        self.poses are updated, the fixed ones stay the same objects' values bit for bit.  No free pose: returns at once (0 iterations,
        converged, chi2 evaluated)."""
        X = [p.copy() for p in self.poses]
        N = len(X)
        H, g, chi2 = self.normal_equations(X)
        free = self.free_index(N)
        out = dict(iterations=0, accepted=0, chi2_initial=chi2, converged=False, chi2_final=chi2, lambda_={**gr.LM_DEFAULTS, **params}["lambda_init"])
        if free.size == 0:
            out["converged"] = True
            return out
        trial = None

        def trials():
            nonlocal trial
            while True:
                d = np.zeros(6 * N)
                d[free] = np.linalg.solve(H[np.ix_(free, free)] + out["lambda_"] * np.eye(free.size), -g[free])
                trial = [X[p].copy() if p in self.fixed else X[p] @ gr.exp(d[6 * p:6 * p + 6]) for p in range(N)]
                yield self.chi2(trial), 0, 0

        for step in gr.lm_decisions(params, chi2, trials()):
            if step["accept"]:
                X = trial
                H, g, _ = self.normal_equations(X)
            out.update(chi2_final=step["chi2"], **{k: step[k] for k in ("lambda_", "converged", "iterations", "accepted")})
        self.poses = X
        return out
