"""Robust kernels on marked between factors, restated in numpy on top of graph_ref: rho and w = rho' of each kind, the
weighted chi2, g and H as dense matrices, and a dense Levenberg-Marquardt that minimises the sum of rho.

Written from the table of include/pcr_hip.h, in its textbook forms (the library evaluates Geman-McClure and Tukey through other, algebraically
equal expressions: the two agree to rounding, not bit for bit).  With s = r^T Omega r and d = delta^2:
    none            rho = s                                               w = 1
    huber           rho = s (s <= d), 2 delta sqrt(s) - d beyond          w = 1, delta / sqrt(s)
    geman_mcclure   rho = d s / (d + s)                                   w = d^2 / (d + s)^2
    tukey           rho = d/3 (1 - (1 - s/d)^3) (s <= d), d/3 beyond      w = (1 - s/d)^2, 0
A marked between factor that is switched on adds rho to chi2, w J^T Omega r to g and w J^T Omega J to H.  Priors and unmarked factors are plain
least squares; a factor that is switched off adds nothing."""
import numpy as np

import graph_ref as gr

NONE, HUBER, GEMAN_MCCLURE, TUKEY = 0, 1, 2, 3
KINDS = {"none": NONE, "huber": HUBER, "geman_mcclure": GEMAN_MCCLURE, "tukey": TUKEY}


def rho_w(kind, delta, s, dtype=np.float64):
    """-> (rho(s), w(s)); dtype=np.longdouble evaluates in extended precision (the derivative test)"""
    s = dtype(s)
    one, two, three = dtype(1), dtype(2), dtype(3)
    if kind == NONE:
        return s, one
    d = dtype(delta) * dtype(delta)
    if kind == HUBER:
        if s <= d:
            return s, one
        q = np.sqrt(s)
        return two * dtype(delta) * q - d, dtype(delta) / q
    if kind == GEMAN_MCCLURE:
        # (d / (d + s) first: the table's d s and (d + s)^2 overflow at s = 1e300)
        q = d / (d + s)
        return q * s, q * q
    if kind == TUKEY:
        if s <= d:
            u = one - s / d
            return d / three * (one - u * u * u), u * u
        return d / three, dtype(0)
    raise ValueError(kind)


class RobustGraph(gr.Graph):
    """graph_ref.Graph plus the kernel (kind, delta), a mark and a switch per between factor."""

    def __init__(self):
        super().__init__()
        self.kind, self.delta = NONE, 0.0
        self.robust, self.enabled = [], []

    def copy(self):
        g = RobustGraph()
        g.poses = [p.copy() for p in self.poses]
        g.priors, g.betweens = list(self.priors), list(self.betweens)
        g.kind, g.delta = self.kind, self.delta
        g.robust, g.enabled = list(self.robust), list(self.enabled)
        return g

    def add_between(self, i, j, Z, Om, robust=False):
        self.betweens.append((i, j, Z, Om))
        self.robust.append(bool(robust))
        self.enabled.append(True)

    def add_loop(self, i, j, Z, Om):
        self.add_between(i, j, Z, Om, robust=True)

    def between_weights(self, poses=None):
        """-> s, w per between factor (w = the kernel's weight at s: 1 when unmarked, whatever the switch says)"""
        X = self.poses if poses is None else poses
        s, w = np.zeros(len(self.betweens)), np.ones(len(self.betweens))
        for e, (i, j, Z, Om) in enumerate(self.betweens):
            r = gr.between_residual(X[i], X[j], Z)
            s[e] = r @ Om @ r
            if self.robust[e]:
                w[e] = rho_w(self.kind, self.delta, s[e])[1]
        return s, w

    def chi2(self, poses=None):
        """the sum of rho over the factors that are switched on"""
        X = self.poses if poses is None else poses
        c = 0.0
        for k, P, Om in self.priors:
            r = gr.prior_residual(X[k], P)
            c += r @ Om @ r
        for e, (i, j, Z, Om) in enumerate(self.betweens):
            if not self.enabled[e]:
                continue
            r = gr.between_residual(X[i], X[j], Z)
            s = r @ Om @ r
            c += rho_w(self.kind, self.delta, s)[0] if self.robust[e] else s
        return float(c)

    def normal_equations(self, poses=None):
        """-> H (6N, 6N) dense, g (6N), chi2 = the sum of rho"""
        X = self.poses if poses is None else poses
        N = len(X)
        r, jf, jt, _ = self.linearize(X)
        H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
        chi2 = 0.0
        for e, (k, _P, Om) in enumerate(self.priors):
            sl = slice(6 * k, 6 * k + 6)
            H[sl, sl] += jt[e].T @ Om @ jt[e]
            g[sl] += jt[e].T @ Om @ r[e]
            chi2 += r[e] @ Om @ r[e]
        P = len(self.priors)
        for b, (i, j, _Z, Om) in enumerate(self.betweens):
            if not self.enabled[b]:
                continue
            e = P + b
            s = r[e] @ Om @ r[e]
            rho, w = rho_w(self.kind, self.delta, s) if self.robust[b] else (s, 1.0)
            chi2 += rho
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            WOm = w * Om
            H[si, si] += jf[e].T @ WOm @ jf[e]
            H[sj, sj] += jt[e].T @ WOm @ jt[e]
            H[si, sj] += jf[e].T @ WOm @ jt[e]
            H[sj, si] += jt[e].T @ WOm @ jf[e]
            g[si] += jf[e].T @ WOm @ r[e]
            g[sj] += jt[e].T @ WOm @ r[e]
        return H, g, float(chi2)

    # optimize() is graph_ref's: it calls normal_equations() and chi2() above, so it minimises the sum of rho by the same accept and stop rules
