"""The pose graph of DESIGN.md 4.17 restated in numpy: SE(3) Exp / Log, the exact Jacobians, prior and between factors, a dense H and
Levenberg-Marquardt with numpy.linalg.solve for the step.  Tangent vectors are [omega; v], rotation first; poses are 4 x 4 matrices.

This is the reference pcr_graph is held to: the same definition, written independently (closed forms with numpy's sin / cos / arccos,
full 6 x 6 adjoint algebra instead of the library's 3 x 3 blocks)."""
import numpy as np

SERIES = 1e-3      # below this angle the coefficient functions are evaluated by their Taylor series


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(t):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3"""
    t2 = t * t
    if t < SERIES:
        return 1 - t2 / 6 + t2 * t2 / 120, 0.5 - t2 / 24 + t2 * t2 / 720, 1 / 6 - t2 / 120 + t2 * t2 / 5040
    return np.sin(t) / t, 2 * np.sin(t / 2) ** 2 / t2, (t - np.sin(t)) / (t2 * t)


def exp(d):
    d = np.asarray(d, dtype=np.float64)
    w, v = d[:3], d[3:]
    t = np.linalg.norm(w)
    A, B, C = _abc(t)
    W = hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W @ W
    T[:3, 3] = (np.eye(3) + B * W + C * W @ W) @ v
    return T


def _log_so3(R):
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(s)
    c = 0.5 * (np.trace(R) - 1.0)
    t = np.arctan2(sn, c)
    if sn < 1e-8 and c > 0:
        return s * (1 + sn * sn / 6)
    if sn < 1e-300:
        return np.zeros(3)
    return s * (t / sn)


def _d_coeff(t):
    """(1 - (t/2) cot(t/2)) / t^2"""
    if t < SERIES:
        return 1 / 12 + t * t / 720 + t ** 4 / 30240
    return (1 - 0.5 * t * np.cos(t / 2) / np.sin(t / 2)) / (t * t)


def log(T):
    w = _log_so3(T[:3, :3])
    t = np.linalg.norm(w)
    W = hat(w)
    Vinv = np.eye(3) - 0.5 * W + _d_coeff(t) * W @ W
    return np.concatenate([w, Vinv @ T[:3, 3]])


def inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def ad(xi):
    a = np.zeros((6, 6))
    a[:3, :3] = hat(xi[:3])
    a[3:, 3:] = hat(xi[:3])
    a[3:, :3] = hat(xi[3:])
    return a


def jr_inv(xi):
    """The inverse right Jacobian of SE(3): ad / (1 - exp(-ad)) = I + ad/2 + a2 ad^2 + a4 ad^4, the even part x/2 coth(x/2) interpolated on
    the spectrum {0, +-i theta (double)} of ad."""
    xi = np.asarray(xi, dtype=np.float64)
    t = np.linalg.norm(xi[:3])
    if t < SERIES:
        a2 = 1 / 12 - t ** 4 / 30240
        a4 = -1 / 720 - 2 * t * t / 30240 - 3 * t ** 4 / 1209600
    else:
        cot = np.cos(t / 2) / np.sin(t / 2)
        gamma = 0.5 * t * cot
        kappa = t / (4 * np.sin(t / 2) ** 2) - 0.5 * cot
        a2 = 2 * (1 - gamma) / t ** 2 - kappa / (2 * t)
        a4 = (1 - gamma) / t ** 4 - kappa / (2 * t ** 3)
    a = ad(xi)
    aa = a @ a
    return np.eye(6) + 0.5 * a + a2 * aa + a4 * aa @ aa


def info_full(info21):
    m = np.zeros((6, 6))
    m[np.triu_indices(6)] = info21
    return m + np.triu(m, 1).T


NOISE = {
    "prior": np.diag(1.0 / np.array([1e-2, 1e-2, np.pi / 72, 1e-1, 1e-1, 1e-1])),
    "odom": np.diag(1.0 / np.array([1e-4, 1e-4, 1e-4, 1e-1, 1e-1, 1e-1])),
    "loop": np.diag(1.0 / np.array([1e-1] * 6)),
}


def between_residual(Xi, Xj, Z):
    return log(inv(Z) @ inv(Xi) @ Xj)


def prior_residual(X, P):
    return log(inv(P) @ X)


def between_jacobians(Xi, Xj, Z):
    """-> r, dr/d(delta_i), dr/d(delta_j) under X <- X Exp(delta)"""
    Tij = inv(Xi) @ Xj
    r = log(inv(Z) @ Tij)
    J = jr_inv(r)
    return r, -J @ adjoint(inv(Tij)), J


def prior_jacobian(X, P):
    r = prior_residual(X, P)
    return r, jr_inv(r)


LM_DEFAULTS = dict(max_iterations=100, rel_tol=1e-5, abs_tol=1e-5, lambda_init=1e-5, lambda_factor=10.0, lambda_max=1e5)


def lm_decisions(params, chi2_0, steps):
    """The Levenberg-Marquardt controller of pcr_graph_optimize (csrc/graph_opt.h) restated: `params` over LM_DEFAULTS, the chi2 of the
    initial estimates, and per trial step (chi2_new, pcg_iterations, pcg_flag).  Yields per step that is taken a dict: accept (the trial
    becomes the estimate), stop, and the state after it -- chi2, lambda_, converged, iterations, accepted, pcg_iterations, pcg_capped.
    `steps` is drawn from only while a trial is wanted, so it may compute each trial from what the last decision left."""
    assert set(params) <= set(LM_DEFAULTS), sorted(set(params) - set(LM_DEFAULTS))
    p = {**LM_DEFAULTS, **params}
    chi2, lam = chi2_0, p["lambda_init"]
    n = dict(converged=False, iterations=0, accepted=0, pcg_iterations=0, pcg_capped=0)
    steps = iter(steps)
    stop = False
    while not stop and n["iterations"] < p["max_iterations"]:
        try:
            c_new, pcg_it, pcg_flag = next(steps)
        except StopIteration:
            return
        n["iterations"] += 1
        n["pcg_iterations"] += pcg_it
        n["pcg_capped"] += 1 if pcg_flag == 1 else 0
        accept = bool(c_new < chi2)
        if accept:
            dec, before = chi2 - c_new, chi2
            chi2 = c_new
            n["accepted"] += 1
            lam /= p["lambda_factor"]
            if dec < p["abs_tol"] or dec < p["rel_tol"] * before:
                n["converged"] = stop = True
        elif c_new - chi2 < p["abs_tol"]:      # could not lower chi2 and raised it by less than abs_tol: at its minimum to that tolerance
            n["converged"] = stop = True
        else:
            lam *= p["lambda_factor"]
            stop = lam > p["lambda_max"]
        yield dict(accept=accept, stop=bool(stop), chi2=chi2, lambda_=lam, **n)


class Graph:
    """priors: (id, P, Omega); betweens: (i, j, Z, Omega); poses: list of 4 x 4."""

    def __init__(self):
        self.poses, self.priors, self.betweens = [], [], []

    def copy(self):
        g = Graph()
        g.poses = [p.copy() for p in self.poses]
        g.priors, g.betweens = list(self.priors), list(self.betweens)
        return g

    def linearize(self, poses=None):
        """-> r (E, 6), J_from (E, 6, 6), J_to (E, 6, 6), chi2; priors first, then the between factors"""
        X = self.poses if poses is None else poses
        E = len(self.priors) + len(self.betweens)
        r, jf, jt = np.zeros((E, 6)), np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
        chi2 = 0.0
        for e, (k, P, Om) in enumerate(self.priors):
            r[e], jt[e] = prior_jacobian(X[k], P)
            chi2 += r[e] @ Om @ r[e]
        for e, (i, j, Z, Om) in enumerate(self.betweens, start=len(self.priors)):
            r[e], jf[e], jt[e] = between_jacobians(X[i], X[j], Z)
            chi2 += r[e] @ Om @ r[e]
        return r, jf, jt, chi2

    def chi2(self, poses=None):
        X = self.poses if poses is None else poses
        c = 0.0
        for k, P, Om in self.priors:
            r = prior_residual(X[k], P)
            c += r @ Om @ r
        for i, j, Z, Om in self.betweens:
            r = between_residual(X[i], X[j], Z)
            c += r @ Om @ r
        return c

    def normal_equations(self, poses=None):
        """-> H (6N, 6N) dense, g (6N), chi2"""
        X = self.poses if poses is None else poses
        N = len(X)
        r, jf, jt, chi2 = self.linearize(X)
        H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
        for e, (k, _P, Om) in enumerate(self.priors):
            s = slice(6 * k, 6 * k + 6)
            H[s, s] += jt[e].T @ Om @ jt[e]
            g[s] += jt[e].T @ Om @ r[e]
        for e, (i, j, _Z, Om) in enumerate(self.betweens, start=len(self.priors)):
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            H[si, si] += jf[e].T @ Om @ jf[e]
            H[sj, sj] += jt[e].T @ Om @ jt[e]
            H[si, sj] += jf[e].T @ Om @ jt[e]
            H[sj, si] += jt[e].T @ Om @ jf[e]
            g[si] += jf[e].T @ Om @ r[e]
            g[sj] += jt[e].T @ Om @ r[e]
        return H, g, chi2

    def optimize(self, **params):
        """Levenberg-Marquardt as pcr_graph_optimize defines it (lm_decisions), the step by a dense solve.  -> dict(iterations, accepted,
        chi2_initial, chi2_final, lambda_, converged); self.poses are updated."""
        X = [p.copy() for p in self.poses]
        N = len(X)
        H, g, chi2 = self.normal_equations(X)
        out = dict(iterations=0, accepted=0, chi2_initial=chi2, converged=False, chi2_final=chi2, lambda_={**LM_DEFAULTS, **params}["lambda_init"])
        trial = None

        def trials():
            nonlocal trial
            while True:
                d = np.linalg.solve(H + out["lambda_"] * np.eye(6 * N), -g)
                trial = [X[p] @ exp(d[6 * p:6 * p + 6]) for p in range(N)]
                yield self.chi2(trial), 0, 0

        for step in lm_decisions(params, chi2, trials()):
            if step["accept"]:
                X = trial
                H, g, _ = self.normal_equations(X)
            out.update(chi2_final=step["chi2"], **{k: step[k] for k in ("lambda_", "converged", "iterations", "accepted")})
        self.poses = X
        return out


def rot_angle(Ra, Rb):
    """the angle of Ra^T Rb"""
    return float(np.linalg.norm(_log_so3(Ra.T @ Rb)))


def pose_diff(A, B):
    """-> (translation distance, rotation angle) between two poses"""
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), rot_angle(A[:3, :3], B[:3, :3])


def random_pose(rng, angle, trans):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    t = rng.uniform(-1, 1, size=3) * trans
    T = exp(np.concatenate([axis * angle, np.zeros(3)]))
    T[:3, 3] = t
    return T
