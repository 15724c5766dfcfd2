"""fast_gicp's Levenberg-Marquardt driver written forwards, in plain Python / numpy float64: LsqRegistration::computeTransformation,
step_lm and is_converged (fast_gicp/optimization/lsq_registration_impl.hpp of the reference project) and so3_exp (so3/so3.hpp), as the
loops they are.  Nothing here comes from csrc/vgicp_opt.h, from the library or from oracle/: tests/test_lm_opt_ref.py holds the
library's pcr_vgicp_opt_* state machine against this module.

The objective is a pair of callbacks: linearize(x0 4x4, k) -> (H 6x6, b 6, e), k = how many trials have been accepted before, and error(xi 4x4, x0 4x4) -> e at xi on the
correspondences of the linearisation at x0.  H is a free input: it need not be the error's Gauss-Newton matrix.

align() returns the final pose, the flag, the number of outer iterations entered, the numbers of linearize and compute_error calls, the
log of trial poses, a census (collections.Counter, LABELS), the largest cond(H + lambda I) of the run and the smallest decision margin
(rho against 0, is_converged's maximum against 1, theta^2 against 1e-10; a comparison with equal sides or a NaN is not counted, as in
tests/ndt_opt_ref.py)."""
import collections
import math

import numpy as np

LABELS = ("rejected_lambda_grown", "inner_exhausted", "converged_on_rejected", "converged_on_accepted", "max_iters_reached", "no_iterations",
          "small_angle", "large_angle", "rho_nan", "lambda_zero", "accepted")


def so3_exp(omega, census=None, note=None):
    """-> quaternion (w, x, y, z)"""
    theta_sq = float(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    if note: note("theta_sq<1e-10", theta_sq, 1e-10)
    if theta_sq < 1e-10:
        theta_quad = theta_sq * theta_sq
        imag_factor = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * theta_quad
        real_factor = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * theta_quad
        if census is not None: census["small_angle"] += 1
    else:
        theta = math.sqrt(theta_sq)
        half_theta = 0.5 * theta
        imag_factor = math.sin(half_theta) / theta
        real_factor = math.cos(half_theta)
        if census is not None: census["large_angle"] += 1
    return real_factor, imag_factor * omega[0], imag_factor * omega[1], imag_factor * omega[2]


def quat_to_matrix(q):
    """Eigen::Quaterniond::toRotationMatrix (the quaternion is used as it is, not normalised)"""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], np.float64)


def ldlt_solve(A, rhs):
    """Eigen::LDLT<Matrix6d>(A).solve(rhs) up to rounding: the solution of the system; rows whose pivot is zero are set to zero, so an
    all-zero matrix gives the zero vector"""
    if not np.any(A):
        return np.zeros(6)
    return np.linalg.solve(A, rhs)


def align(linearize, error, guess, max_iterations, lm_max_iterations, lm_init_lambda_factor, rotation_epsilon, transformation_epsilon):
    census = collections.Counter()
    st = dict(margin=math.inf, margin_at=None, cond=1.0, n_lin=0, n_err=0, lm_lambda=-1.0)
    trials = []

    def note(what, a, b):
        if a == b or a != a or b != b or math.isinf(a) or math.isinf(b):
            return
        m = abs(a - b) / max(abs(a), abs(b))
        if m < st["margin"]:
            st["margin"], st["margin_at"] = m, what

    def is_converged(delta):
        R = delta[:3, :3] - np.eye(3)
        t = delta[:3, 3]
        r_delta = 1.0 / rotation_epsilon * np.abs(R)
        t_delta = 1.0 / transformation_epsilon * np.abs(t)
        v = max(float(r_delta.max()), float(t_delta.max()))
        note("is_converged", v, 1.0)
        return v < 1

    def step_lm(x0):
        """-> (ok, x0, delta)"""
        H, b, y0 = linearize(x0.copy(), census["accepted"])
        H = np.array(H, np.float64).reshape(6, 6); b = np.array(b, np.float64).reshape(6); y0 = float(y0)
        st["n_lin"] += 1
        if st["lm_lambda"] < 0.0:
            st["lm_lambda"] = lm_init_lambda_factor * float(np.abs(np.diag(H)).max())
            if st["lm_lambda"] == 0: census["lambda_zero"] += 1
        nu = 2.0
        delta = np.eye(4)
        for i in range(lm_max_iterations):
            A = H + st["lm_lambda"] * np.eye(6)
            if np.any(A) and np.all(np.isfinite(A)):
                st["cond"] = max(st["cond"], float(np.linalg.cond(A)))
            d = ldlt_solve(A, -b)
            delta = np.eye(4)
            delta[:3, :3] = quat_to_matrix(so3_exp(d[:3], census, note))
            delta[:3, 3] = d[3:]
            xi = np.eye(4)
            xi[:3, :3] = delta[:3, :3] @ x0[:3, :3]
            xi[:3, 3] = delta[:3, :3] @ x0[:3, 3] + delta[:3, 3]
            trials.append(xi.copy())
            yi = float(error(xi.copy(), x0.copy()))
            st["n_err"] += 1
            with np.errstate(all="ignore"):
                rho = float((np.float64(y0) - np.float64(yi)) / np.float64(d @ (st["lm_lambda"] * d - b)))
            if rho != rho: census["rho_nan"] += 1
            note("rho<0", y0, yi)
            if rho < 0:
                if is_converged(delta):
                    census["converged_on_rejected"] += 1
                    return True, x0, delta
                st["lm_lambda"] = nu * st["lm_lambda"]
                nu = 2 * nu
                census["rejected_lambda_grown"] += 1
                continue
            x0 = xi
            f = 1 - (2 * rho - 1) ** 3
            st["lm_lambda"] = st["lm_lambda"] * (f if 1.0 / 3.0 < f else 1.0 / 3.0)      # std::max(1.0 / 3.0, f): a NaN f gives 1/3
            census["accepted"] += 1
            return True, x0, delta
        census["inner_exhausted"] += 1
        return False, x0, delta

    x0 = np.array(guess, np.float32).astype(np.float64)      # guess.cast<double>() of a Matrix4f
    converged, entered = False, 0
    i = 0
    if max_iterations <= 0: census["no_iterations"] += 1
    while i < max_iterations and not converged:
        entered = i + 1
        ok, x0, delta = step_lm(x0)
        if not ok:
            break
        converged = is_converged(delta)
        if converged and not census["converged_on_rejected"]: census["converged_on_accepted"] += 1
        i += 1
        if i >= max_iterations and not converged: census["max_iters_reached"] += 1
    return dict(pose=x0, converged=bool(converged), outer=entered, n_lin=st["n_lin"], n_err=st["n_err"], trials=trials, census=census,
                cond=st["cond"], margin=st["margin"], margin_at=st["margin_at"])


# ---- objectives ----------------------------------------------------------------------------------------------------------------------
def pose_from(rot, t):
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(so3_exp(np.asarray(rot, np.float64)))
    T[:3, 3] = t
    return T


def xi_of(T):
    """six coordinates of a pose: the skew part of R (the rotation vector to first order) and the translation"""
    R = T[:3, :3]
    return np.array([0.5 * (R[2, 1] - R[1, 2]), 0.5 * (R[0, 2] - R[2, 0]), 0.5 * (R[1, 0] - R[0, 1]), T[0, 3], T[1, 3], T[2, 3]])


def quadratic(A, target, h_scale=1.0):
    """e(T) = 0.5 r' A r with r = xi_of(T) - xi_of(target); b = A r; the fed H = h_scale * A (a small h_scale makes the steps overshoot
    and the trials fail).  The error does not depend on the correspondences."""
    A = np.asarray(A, np.float64); x_star = xi_of(target)

    def e(T):
        r = xi_of(T) - x_star
        return 0.5 * float(r @ A @ r)

    def linearize(x0, k):
        r = xi_of(x0) - x_star
        return h_scale * A, A @ r, e(x0)

    def error(xi, x0):
        return e(xi)
    return linearize, error


def scripted(lins, errs):
    """linearize returns lins[k] = (H, b, e) for the pose after k accepted trials, error errs[j] at its j-th call (the last entry stays)"""
    n = dict(e=0)

    def linearize(x0, k):
        H, b, e = lins[min(k, len(lins) - 1)]
        return np.array(H, np.float64), np.array(b, np.float64), float(e)

    def error(xi, x0):
        k = min(n["e"], len(errs) - 1); n["e"] += 1
        return float(errs[k])
    return linearize, error
