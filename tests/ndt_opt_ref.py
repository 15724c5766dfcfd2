"""pclomp's NDT optimiser written forwards, in plain Python / numpy float64: NormalDistributionsTransform::computeTransformation,
computeStepLengthMT, trialValueSelectionMT, updateIntervalMT and the two auxiliary functions (third_parties/pclomp/src/ndt_omp_impl.hpp
of the reference project), as the nested loops they are.  Nothing here comes from csrc/ndt_opt.h, from the library or from oracle/: this
module is what tests/test_ndt_opt_ref.py and tests/test_ndt_opt_gpu.py hold the library's state machine against.

The objective is a callback f(p6, want) -> (score, grad[6], hess[36]); want is "dh" (computeDerivatives with the Hessian), "d"
(computeDerivatives without: the loop zeroes the Hessian itself, as the reference does) or "h" (computeHessian).  The Hessian that is fed
is a free input: it need not be the score's.

align() returns the final p, the flag, nr_iterations, the number of computeDerivatives and computeHessian calls, the log of every
evaluation in order, a census of the branches taken (collections.Counter, labels in LABELS) and the smallest decision margin of the run.

Decision margin: for every comparison that takes a decision, the distance of its two sides relative to the scale its operands live on
(function values: |phi'(0)| * step; slopes: |phi'(0)|; steps: the larger step).  Two Newton solves that differ in the last bit (Jacobi SVD,
LAPACK SVD, an LU) move every quantity of a search by ~cond * eps of that scale, so a run whose smallest margin is far above that takes the
same branches with either solve.  A comparison whose two sides are EQUAL, or of which one is NaN, is not counted: such ties are not the
work of rounding -- they are copies of one number (a trial clamped to step_max compared with the a_l that was set from the same clamped
trial) or designed inputs (a zero gradient), and both solves see them alike.
"""
import collections
import ctypes
import ctypes.util
import math

import numpy as np

F32 = np.float32
EPS = 2.220446049250313e-16

LABELS = (
    # trialValueSelectionMT: seven outcomes, case 3's clamp as labels of its own
    "tv1_cubic", "tv1_average", "tv2_cubic", "tv2_secant", "tv3_cubic", "tv3_secant", "tv3_min", "tv3_max", "tv4",
    # updateIntervalMT
    "ui_u1", "ui_u2", "ui_u3", "ui_converged",
    "interval_closed", "trial_on_closed",
    "end_cap", "end_interval_converged", "end_wolfe_first", "end_wolfe_later",
    "dir_flipped", "dphi0_zero", "nrm_zero", "nrm_nan",
    "clamp_high", "clamp_low", "trial_repeat",
)
# what a run of repeated trial points (a_t equal to the previous trial: the evaluations the library answers itself) passes through
REPEAT_LABELS = ("repeat_closes_interval", "repeat_ends_by_cap", "repeat_ends_by_ui_converged", "repeat_ends_by_wolfe", "repeat_then_new_point")


def std_min(a, b):
    """std::min(a, b): (b < a) ? b : a -- a NaN in b is dropped, a NaN in a is kept"""
    return b if b < a else a


def std_max(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return b if a < b else a


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]


def sinf(x):
    return F32(_libm.sinf(float(F32(x))))


def cosf(x):
    return F32(_libm.cosf(float(F32(x))))


def _angle_axis(angle, axis):
    """Eigen::AngleAxisf(angle, Unit{X,Y,Z}).toRotationMatrix(): every operation in float, rounded"""
    ax = np.zeros(3, F32)
    ax[axis] = F32(1)
    s, c = sinf(angle), cosf(angle)
    sin_axis = [s * ax[i] for i in range(3)]
    cos1_axis = [(F32(1) - c) * ax[i] for i in range(3)]
    R = np.zeros((3, 3), F32)
    tmp = cos1_axis[0] * ax[1]; R[0, 1] = tmp - sin_axis[2]; R[1, 0] = tmp + sin_axis[2]
    tmp = cos1_axis[0] * ax[2]; R[0, 2] = tmp + sin_axis[1]; R[2, 0] = tmp - sin_axis[1]
    tmp = cos1_axis[1] * ax[2]; R[1, 2] = tmp - sin_axis[0]; R[2, 1] = tmp + sin_axis[0]
    for d in range(3):
        R[d, d] = cos1_axis[d] * ax[d] + c
    return R


def _mul33(A, B):
    C = np.zeros((3, 3), F32)
    for r in range(3):
        for c in range(3):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            C[r, c] = s
    return C


def float_pose(x):
    """(Translation3f(x[0:3]) * AngleAxisf(x[3], X) * AngleAxisf(x[4], Y) * AngleAxisf(x[5], Z)).matrix() -> 4x4 float32"""
    with np.errstate(all="ignore"):
        R = _mul33(_mul33(_angle_axis(F32(x[3]), 0), _angle_axis(F32(x[4]), 1)), _angle_axis(F32(x[5]), 2))
    T = np.zeros((4, 4), F32)
    T[:3, :3] = R
    T[:3, 3] = [F32(x[0]), F32(x[1]), F32(x[2])]
    T[3, 3] = F32(1)
    return T


def angle_tables(p, sin=math.sin, cos=math.cos):
    """computeAngleDerivatives -> (j float32 [8,3], h float32 [15,3], jd float64 [8,3], hd float64 [15,3]): the j_ang / h_ang matrices the
    point loops use (their fourth column is zero) and the double vectors j_ang_a_ .. h_ang_f3_"""
    def sc(a):
        if math.fabs(a) < 10e-5:
            return 0.0, 1.0
        return sin(a), cos(a)
    sx, cx = sc(p[3]); sy, cy = sc(p[4]); sz, cz = sc(p[5])
    jd = np.array([
        [(-sx * sz + cx * sy * cz), (-sx * cz - cx * sy * sz), (-cx * cy)],
        [(cx * sz + sx * sy * cz), (cx * cz - sx * sy * sz), (-sx * cy)],
        [(-sy * cz), sy * sz, cy],
        [sx * cy * cz, (-sx * cy * sz), sx * sy],
        [(-cx * cy * cz), cx * cy * sz, (-cx * sy)],
        [(-cy * sz), (-cy * cz), 0],
        [(cx * cz - sx * sy * sz), (-cx * sz - sx * sy * cz), 0],
        [(sx * cz + cx * sy * sz), (cx * sy * cz - sx * sz), 0]], np.float64)
    hd = np.array([
        [(-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), sx * cy],
        [(-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), (-cx * cy)],
        [(cx * cy * cz), (-cx * cy * sz), (cx * sy)],
        [(sx * cy * cz), (-sx * cy * sz), (sx * sy)],
        [(-sx * cz - cx * sy * sz), (sx * sz - cx * sy * cz), 0],
        [(cx * cz - sx * sy * sz), (-sx * sy * cz - cx * sz), 0],
        [(-cy * cz), (cy * sz), (-sy)],
        [(-sx * sy * cz), (sx * sy * sz), (sx * cy)],
        [(cx * sy * cz), (-cx * sy * sz), (-cx * cy)],
        [(sy * sz), (sy * cz), 0],
        [(-sx * cy * sz), (-sx * cy * cz), 0],
        [(cx * cy * sz), (cx * cy * cz), 0],
        [(-cy * cz), (cy * sz), 0],
        [(-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), 0],
        [(-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), 0]], np.float64)
    j = jd.astype(F32)
    h = hd.astype(F32)
    h[6, 2] = F32(sy)      # h_ang.row(6) is written with (sy) where h_ang_d1_ has (-sy)
    return j, h, jd, hd


def svd_solve(H, b):
    """Eigen::JacobiSVD<Matrix6d>(H, ComputeFullU | ComputeFullV).solve(b): pseudo-inverse, singular values up to
    6 * eps * sigma_max dropped (Eigen's default threshold: diagSize * epsilon)"""
    H = np.asarray(H, np.float64).reshape(6, 6)
    if not np.all(np.isfinite(H)):      # Eigen >= 3.4: compute() finds the largest entry not finite, reports InvalidInput with rank 0: solve() returns zero
        return np.zeros(6)
    U, s, Vt = np.linalg.svd(H)
    thr = 6.0 * EPS * s[0]
    x = np.zeros(6)
    for k in range(6):
        if s[k] > thr:
            x = x + Vt[k] * (float(U[:, k] @ b) / s[k])
    return x


class _Run:
    def __init__(self, f):
        self.f = f
        self.census = collections.Counter()
        self.margin = math.inf
        self.margin_at = None
        self.log = []            # (kind, p6) of every evaluation, kind in "dh", "d", "h"
        self.log_x = []          # for every log entry: the point the search it belongs to started from (the point itself for the first)
        self.x = None
        self.moves = []          # (p6, float pose) of every trial point, in order
        self.n_deriv = self.n_hess = 0

    def cmp(self, what, a, b, scale):
        """records how close the comparison of a with b is (see the module docstring)"""
        if a == b or a != a or b != b or math.isinf(a) or math.isinf(b):
            return
        scale = max(abs(a), abs(b), abs(scale)) if scale == scale and not math.isinf(scale) else max(abs(a), abs(b))
        m = abs(a - b) / scale
        if m < self.margin:
            self.margin, self.margin_at = m, what

    def derivatives(self, p, with_hessian):
        score, grad, hess = self.f(np.array(p, np.float64), "dh" if with_hessian else "d")
        self.log.append(("dh" if with_hessian else "d", np.array(p, np.float64)))
        self.log_x.append(np.array(p if self.x is None else self.x, np.float64))
        self.n_deriv += 1
        hess = np.array(hess, np.float64).reshape(36) if with_hessian else np.zeros(36)
        return float(score), np.array(grad, np.float64).reshape(6), hess

    def hessian(self, p):
        _, _, hess = self.f(np.array(p, np.float64), "h")
        self.log.append(("h", np.array(p, np.float64)))
        self.log_x.append(np.array(self.x, np.float64))
        self.n_hess += 1
        return np.array(hess, np.float64).reshape(36)


def aux_psi(a, f_a, f_0, g_0, mu):
    return f_a - f_0 - mu * g_0 * a


def aux_dpsi(g_a, g_0, mu):
    return g_a - mu * g_0


def update_interval(run, I, a_t, f_t, g_t, fs, gs):
    """updateIntervalMT on I = [a_l, f_l, g_l, a_u, f_u, g_u] (in place) -> converged"""
    a_l, f_l, g_l = I[0], I[1], I[2]
    run.cmp("ui f_t>f_l", f_t, f_l, fs)
    if f_t > f_l:
        I[3], I[4], I[5] = a_t, f_t, g_t
        run.census["ui_u1"] += 1
        return False
    run.cmp("ui g_t sign", g_t, 0.0, gs)
    run.cmp("ui a_l-a_t sign", a_l, a_t, 0.0)
    if g_t * (a_l - a_t) > 0:
        I[0], I[1], I[2] = a_t, f_t, g_t
        run.census["ui_u2"] += 1
        return False
    if g_t * (a_l - a_t) < 0:
        I[3], I[4], I[5] = a_l, f_l, g_l
        I[0], I[1], I[2] = a_t, f_t, g_t
        run.census["ui_u3"] += 1
        return False
    run.census["ui_converged"] += 1
    return True


def trial_value(run, I, a_t, f_t, g_t, fs, gs):
    """trialValueSelectionMT"""
    a_l, f_l, g_l, a_u, f_u, g_u = (np.float64(v) for v in I)      # numpy scalars: x / 0 is inf or NaN, as in C
    a_t, f_t, g_t = np.float64(a_t), np.float64(f_t), np.float64(g_t)
    with np.errstate(all="ignore"):
        run.cmp("tv f_t>f_l", f_t, f_l, fs)
        if f_t > f_l:
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = _sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t))
            run.cmp("tv1 |a_c-a_l|<|a_q-a_l|", abs(a_c - a_l), abs(a_q - a_l), a_t)
            if abs(a_c - a_l) < abs(a_q - a_l):
                run.census["tv1_cubic"] += 1
                return float(a_c)
            run.census["tv1_average"] += 1
            return float(0.5 * (a_q + a_c))
        run.cmp("tv g_t sign", g_t, 0.0, gs)
        if g_t * g_l < 0:
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = _sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
            run.cmp("tv2 |a_c-a_t|>=|a_s-a_t|", abs(a_c - a_t), abs(a_s - a_t), a_t)
            if abs(a_c - a_t) >= abs(a_s - a_t):
                run.census["tv2_cubic"] += 1
                return float(a_c)
            run.census["tv2_secant"] += 1
            return float(a_s)
        run.cmp("tv |g_t|<=|g_l|", abs(g_t), abs(g_l), gs)
        if abs(g_t) <= abs(g_l):
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = _sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
            run.cmp("tv3 |a_c-a_t|<|a_s-a_t|", abs(a_c - a_t), abs(a_s - a_t), a_t)
            if abs(a_c - a_t) < abs(a_s - a_t):
                run.census["tv3_cubic"] += 1
                a_t_next = a_c
            else:
                run.census["tv3_secant"] += 1
                a_t_next = a_s
            run.cmp("tv3 a_t>a_l", a_t, a_l, 0.0)
            lim = a_t + 0.66 * (a_u - a_t)
            run.cmp("tv3 clamp", lim, a_t_next, a_t)
            if a_t > a_l:
                run.census["tv3_min"] += 1
                return float(std_min(lim, a_t_next))
            run.census["tv3_max"] += 1
            return float(std_max(lim, a_t_next))
        run.census["tv4"] += 1
        z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u
        w = _sqrt(z * z - g_t * g_u)
        return float(a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w))


def _sqrt(v):
    v = float(v)
    return math.sqrt(v) if v >= 0 else math.nan      # std::sqrt of a negative number, or of NaN, is NaN


def step_length_mt(run, x, step_dir, step_init, step_max, step_min, st):
    """computeStepLengthMT.  st: dict(score, grad, hess, final) updated in place, step_dir flipped in place.  -> a_t"""
    run.x = np.array(x, np.float64)
    phi_0 = -st["score"]
    d_phi_0 = -float(_dot(st["grad"], step_dir))
    run.cmp("d_phi_0>=0", d_phi_0, 0.0, float(np.sum(np.abs(st["grad"] * step_dir))))
    if d_phi_0 >= 0:
        if d_phi_0 == 0:
            run.census["dphi0_zero"] += 1
            return 0.0
        d_phi_0 *= -1
        step_dir *= -1
        run.census["dir_flipped"] += 1
    max_step_iterations, step_iterations = 10, 0
    mu, nu = 1.e-4, 0.9
    a_l = a_u = 0.0
    f_l = aux_psi(a_l, phi_0, phi_0, d_phi_0, mu); g_l = aux_dpsi(d_phi_0, d_phi_0, mu)
    f_u = aux_psi(a_u, phi_0, phi_0, d_phi_0, mu); g_u = aux_dpsi(d_phi_0, d_phi_0, mu)
    I = [a_l, f_l, g_l, a_u, f_u, g_u]
    interval_converged, open_interval = (step_max - step_min) < 0, True
    a_t = step_init
    run.cmp("clamp high", a_t, step_max, 0.0); run.cmp("clamp low", a_t, step_min, 0.0)
    if step_max < a_t: run.census["clamp_high"] += 1
    a_t = std_min(a_t, step_max)
    if a_t < step_min: run.census["clamp_low"] += 1
    a_t = std_max(a_t, step_min)
    x_t = x + step_dir * a_t
    st["final"] = float_pose(x_t)
    run.moves.append((x_t.copy(), st["final"]))
    st["score"], st["grad"], st["hess"] = run.derivatives(x_t, True)
    phi_t = -st["score"]
    d_phi_t = -float(_dot(st["grad"], step_dir))
    psi_t = aux_psi(a_t, phi_t, phi_0, d_phi_0, mu)
    d_psi_t = aux_dpsi(d_phi_t, d_phi_0, mu)
    gs = abs(d_phi_0)
    repeat = False      # the last evaluation was at the point of the one before
    while True:
        fs = abs(d_phi_0) * max(abs(a_t), abs(I[0]))
        if interval_converged:
            run.census["end_interval_converged"] += 1
            if repeat: run.census["repeat_ends_by_ui_converged"] += 1
            break
        if not step_iterations < max_step_iterations:
            run.census["end_cap"] += 1
            if repeat: run.census["repeat_ends_by_cap"] += 1
            break
        run.cmp("wolfe psi_t<=0", psi_t, 0.0, fs); run.cmp("wolfe curvature", d_phi_t, -nu * d_phi_0, gs)
        if psi_t <= 0 and d_phi_t <= -nu * d_phi_0:
            run.census["end_wolfe_later" if step_iterations else "end_wolfe_first"] += 1
            if repeat: run.census["repeat_ends_by_wolfe"] += 1
            break
        a_prev = a_t
        if open_interval:
            a_t = trial_value(run, I, a_t, psi_t, d_psi_t, fs, gs)
        else:
            run.census["trial_on_closed"] += 1
            a_t = trial_value(run, I, a_t, phi_t, d_phi_t, fs, gs)
        run.cmp("clamp high", a_t, step_max, 0.0); run.cmp("clamp low", a_t, step_min, 0.0)
        if step_max < a_t: run.census["clamp_high"] += 1
        a_t = std_min(a_t, step_max)
        if a_t < step_min: run.census["clamp_low"] += 1
        a_t = std_max(a_t, step_min)
        if repeat and a_t != a_prev: run.census["repeat_then_new_point"] += 1
        repeat = a_t == a_prev
        if repeat: run.census["trial_repeat"] += 1
        x_t = x + step_dir * a_t
        st["final"] = float_pose(x_t)
        run.moves.append((x_t.copy(), st["final"]))
        st["score"], st["grad"], st["hess"] = run.derivatives(x_t, False)
        phi_t = -st["score"]
        d_phi_t = -float(_dot(st["grad"], step_dir))
        psi_t = aux_psi(a_t, phi_t, phi_0, d_phi_0, mu)
        d_psi_t = aux_dpsi(d_phi_t, d_phi_0, mu)
        fs = abs(d_phi_0) * max(abs(a_t), abs(I[0]))
        if open_interval:
            run.cmp("close psi_t<=0", psi_t, 0.0, fs); run.cmp("close d_psi_t>=0", d_psi_t, 0.0, gs)
        if open_interval and (psi_t <= 0 and d_psi_t >= 0):
            open_interval = False
            run.census["interval_closed"] += 1
            if repeat: run.census["repeat_closes_interval"] += 1
            I[1] = I[1] + phi_0 - mu * d_phi_0 * I[0]
            I[2] = I[2] + mu * d_phi_0
            I[4] = I[4] + phi_0 - mu * d_phi_0 * I[3]
            I[5] = I[5] + mu * d_phi_0
        if open_interval:
            interval_converged = update_interval(run, I, a_t, psi_t, d_psi_t, fs, gs)
        else:
            interval_converged = update_interval(run, I, a_t, phi_t, d_phi_t, fs, gs)
        step_iterations += 1
    if step_iterations:
        st["hess"] = run.hessian(x_t)
    st["a_t_last"] = a_t
    return a_t


def _dot(a, b):
    s = 0.0
    for i in range(6):
        s += float(a[i]) * float(b[i])
    return s


def align(f, p0, step_size, trans_eps, max_iters, T0=None):
    """computeTransformation from the 6-vector p0 (T0: the float guess final_transformation_ starts as; float_pose(p0) if not given).
    -> dict(p, converged, iterations, n_deriv, n_hess, log, moves, census, margin, margin_at, pose, steps)"""
    run = _Run(f)
    p = np.array(p0, np.float64)
    st = dict(final=float_pose(p) if T0 is None else np.array(T0, F32))
    nr_iterations, converged = 0, False
    steps = []      # the step length every Newton iteration ended with
    st["score"], st["grad"], st["hess"] = run.derivatives(p, True)
    while not converged:
        delta_p = svd_solve(st["hess"], -st["grad"])
        delta_p_norm = math.sqrt(_dot(delta_p, delta_p))
        if delta_p_norm == 0 or delta_p_norm != delta_p_norm:
            run.census["nrm_zero" if delta_p_norm == 0 else "nrm_nan"] += 1
            converged = delta_p_norm == delta_p_norm
            break
        delta_p = delta_p / delta_p_norm
        delta_p_norm = step_length_mt(run, p, delta_p, delta_p_norm, step_size, trans_eps / 2, st)
        steps.append(delta_p_norm)
        delta_p = delta_p * delta_p_norm
        p = p + delta_p
        run.cmp("|delta_p_norm|<trans_eps", abs(delta_p_norm), trans_eps, 0.0)
        if nr_iterations > max_iters or (nr_iterations and abs(delta_p_norm) < trans_eps):
            converged = True
        nr_iterations += 1
    return dict(p=p, converged=bool(converged), iterations=nr_iterations, n_deriv=run.n_deriv, n_hess=run.n_hess, log=run.log, log_x=run.log_x,
                moves=run.moves, census=run.census, margin=run.margin, margin_at=run.margin_at, pose=st["final"], steps=steps)


# ---- objective families ------------------------------------------------------------------------------------------------------------
def spd_with_condition(rng, cond):
    """a symmetric positive definite 6x6 matrix with eigenvalues spread geometrically over [1, cond]"""
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    return (Q * np.geomspace(1.0, cond, 6)) @ Q.T


def quadratic(A, c, hess_scale=1.0, ripple=0.0, freq=None):
    """score(p) = -(0.5 (p-c)' A (p-c) + ripple * sum_i (1 - cos(freq_i . (p-c)))): a maximum at c.  The Hessian that is fed is
    hess_scale * the quadratic's (-A): the ripple's curvature is left out, and a scale other than 1 makes the Newton step too long, too
    short or point uphill."""
    A = np.asarray(A, np.float64); c = np.asarray(c, np.float64)
    freq = np.zeros((0, 6)) if freq is None else np.asarray(freq, np.float64)
    Hfed = (-A * hess_scale).reshape(36)

    def f(p, want):
        d = p - c
        ph = freq @ d
        score = -(0.5 * d @ A @ d + ripple * float(np.sum(1 - np.cos(ph))))
        grad = -(A @ d + ripple * (freq.T @ np.sin(ph)))
        return score, grad, Hfed
    return f


def profile_1d(u, base, g, dg, h_u, stiff=50.0):
    """score(p) = -(g(a) + 0.5 * stiff * |perp|^2), a = u . (p - base), perp = the rest: a 1-D profile g along the unit vector u with the
    other five directions stiff.  The fed Hessian is -(h_u(a) u u' + stiff (I - u u')): the Newton step is dg(a) / h_u(a) along u."""
    u = np.asarray(u, np.float64); u = u / np.linalg.norm(u); base = np.asarray(base, np.float64)
    P = np.eye(6) - np.outer(u, u)

    def f(p, want):
        d = p - base
        a = float(u @ d)
        perp = P @ d
        score = -(g(a) + 0.5 * stiff * float(perp @ perp))
        grad = -(dg(a) * u + stiff * perp)
        H = -(h_u(a) * np.outer(u, u) + stiff * P)
        return score, grad, H.reshape(36)
    return f


def scripted(entries):
    """Returns entry k = (score, grad, hess) at the k-th DISTINCT point it is asked at, whatever that point is: asking again at the point
    of the previous call (a repeated trial, a Hessian at the last trial point) repeats the entry.  Past the end the last entry stays."""
    state = dict(k=-1, p=None)

    def f(p, want):
        if state["p"] is None or not np.array_equal(p, state["p"], equal_nan=True):
            state["k"] = min(state["k"] + 1, len(entries) - 1)
            state["p"] = p.copy()
        s, g, H = entries[state["k"]]
        return float(s), np.array(g, np.float64), np.array(H, np.float64).reshape(36)
    return f
