"""csrc/vgicp_opt.h on the host (pcr_vgicp_opt_*) against tests/lm_opt_ref.py, the reference's LsqRegistration::computeTransformation /
step_lm / is_converged / so3_exp written forwards: the same callbacks drive both, and the state machine must take the reference's
decisions -- same flag, outer iterations, linearize and compute_error counts -- and arrive at its poses.

Tolerance.  Both sides do the same double arithmetic on the same sums except the 6x6 solve of (H + lambda I) d = -b (the library restates
Eigen's LDLT, the reference module calls LAPACK): each d carries c * cond(H + lambda I) * eps * |d| with c ~ n^2 = 36 for a backward-stable
solve, a run accepts at most max_iters <= 30 steps whose errors add, and the objective is evaluated at the perturbed pose (a contraction
for the families here): 36 * 30 ~ 1e3.  So every trial pose and the final pose must agree within
    LM_FACTOR * cond_max * eps * max(1, |entry|_max),   LM_FACTOR = 1e3,
cond_max = the largest cond(H + lambda I) the reference met in the run.  A case qualifies if its smallest decision margin (rho against 0,
is_converged's maximum against 1, theta^2 against 1e-10) exceeds 1e-6, seven orders above cond * eps for cond <= 1e3."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

import lm_opt_ref as R
from simpleslam_amd.pcr import load_library

DP = C.POINTER(C.c_double)
IU = np.triu_indices(6)
EPS = 2.220446049250313e-16
LM_FACTOR = 1e3
MARGIN_MIN = 1e-6


def c16(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16).copy()


def drive(L, case):
    linearize, error = case["make"]()
    g = c16(case["guess"])
    o = L.pcr_vgicp_opt_create(g.ctypes.data_as(DP), int(case["max_iters"]), int(case["lm_inner"]), float(case["lm_init"]), float(case["rot_eps"]),
                               float(case["trans_eps"]))
    assert o
    try:
        trials, n_lin, n_err, accepted, lin_prev = [], 0, 0, 0, None
        for _ in range(5000):
            kind, pe, pl = C.c_int(-1), np.zeros(16), np.zeros(16)
            assert L.pcr_vgicp_opt_request(o, C.byref(kind), pe.ctypes.data_as(DP), pl.ctypes.data_as(DP)) == 0
            if kind.value == 2:
                break
            Te, Tl = pe.reshape(4, 4).T.copy(), pl.reshape(4, 4).T.copy()
            if lin_prev is not None and not np.array_equal(Tl, lin_prev):
                accepted += 1      # (the linearisation point moved: the last trial was accepted)
            lin_prev = Tl
            sums = np.zeros(29)
            # a trial pass linearises AT the trial pose: the linearisation the reference computes next if the trial is accepted
            H, b, e = linearize(Te, accepted + (1 if kind.value == 1 else 0))
            sums[:21] = np.asarray(H).reshape(6, 6)[IU]; sums[21:27] = b; sums[27] = e
            if kind.value == 1:
                sums[28] = error(Te, Tl)
                trials.append(Te)
                n_err += 1
            assert L.pcr_vgicp_opt_feed(o, sums.ctypes.data_as(DP)) == 0
        else:
            raise AssertionError("the optimiser did not finish")
        pose, conv, outer, done = np.zeros(16), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.pcr_vgicp_opt_result(o, pose.ctypes.data_as(DP), C.byref(conv), C.byref(outer), C.byref(done)) == 0 and done.value == 1
        assert L.pcr_vgicp_opt_feed(o, np.zeros(29).ctypes.data_as(DP)) == 1      # a feed after done is refused
        return dict(pose=pose.reshape(4, 4).T.copy(), converged=bool(conv.value), outer=outer.value, n_err=n_err, trials=trials)
    finally:
        L.pcr_vgicp_opt_destroy(o)


def reference(case):
    linearize, error = case["make"]()
    return R.align(linearize, error, case["guess"], case["max_iters"], case["lm_inner"], case["lm_init"], case["rot_eps"], case["trans_eps"])


def spd(rng, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    return (Q * np.geomspace(1.0, cond, 6)) @ Q.T


def random_cases():
    out = []
    for seed in range(40):
        rng = np.random.default_rng(300 + seed)
        A = spd(rng, (10.0, 100.0, 1000.0)[seed % 3])
        target = R.pose_from(rng.normal(0, 0.2, 3), rng.normal(0, 1.0, 3))
        guess = R.pose_from(rng.normal(0, 0.2, 3) + rng.normal(0, 0.05, 3), rng.normal(0, 1.0, 3)).astype(np.float32).astype(np.float64)
        guess[:3, 3] = target[:3, 3] + rng.normal(0, 0.3, 3)
        guess = guess.astype(np.float32).astype(np.float64)
        for h_scale in (1.0, 0.3, 0.05):        # 0.05: steps 20 times too long: rejected until lambda has grown
            for max_iters, lm_inner, eps in ((30, 10, (2e-3, 5e-4)), (3, 10, (2e-3, 5e-4)), (30, 3, (2e-3, 5e-4)), (30, 10, (1e-9, 1e-9))):
                out.append(dict(name=f"quad-s{seed}-h{h_scale}-m{max_iters}-i{lm_inner}-e{eps[0]}", guess=guess, max_iters=max_iters, lm_inner=lm_inner,
                                lm_init=1e-9, rot_eps=eps[0], trans_eps=eps[1], make=lambda A=A, t=target, h=h_scale: R.quadratic(A, t, h)))
    return out


def designed_cases():
    I6 = np.eye(6)
    g = np.eye(4); g[:3, 3] = (0.5, -0.25, 1.0)
    base = dict(guess=g, max_iters=5, lm_inner=10, lm_init=1e-9, rot_eps=2e-3, trans_eps=5e-4)
    b1 = np.array([1e-5, 0, 0, 1e-5, 0, 0])
    out = [
        dict(base, name="max-iters-zero", max_iters=0, make=lambda: R.scripted([(I6, b1, 1.0)], [0.5])),
        dict(base, name="max-iters-negative", max_iters=-3, make=lambda: R.scripted([(I6, b1, 1.0)], [0.5])),
        # a tiny step whose error is worse: rho < 0 and the step is below both epsilons: converged, x0 untouched
        dict(base, name="converged-on-rejected", make=lambda: R.scripted([(I6, b1, 1.0)], [2.0])),
        # every trial worse and the step large: lambda 1e-9 * (2, 8, 64): given up after lm_inner trials
        dict(base, name="inner-exhausted", lm_inner=3, make=lambda: R.scripted([(I6, np.full(6, 0.1), 1.0)], [2.0])),
        # b = 0: d = 0, den = 0, y0 == yi: rho is NaN, which is not < 0: the trial is ACCEPTED, lambda *= std::max(1/3, NaN) = 1/3, converged
        dict(base, name="rho-nan", make=lambda: R.scripted([(I6, np.zeros(6), 1.0)], [1.0])),
        # an all-zero first linearisation: lambda = 1e-9 * 0 = 0, the solve of the zero matrix gives d = 0
        dict(base, name="lambda-zero", make=lambda: R.scripted([(np.zeros((6, 6)), np.zeros(6), 1.0)], [1.0])),
        # so3_exp either side of theta^2 = 1e-10: rotation steps of 0.9e-5 and 1.1e-5 rad
        dict(base, name="theta-below", rot_eps=1e-9, trans_eps=1e-9, max_iters=1, make=lambda: R.scripted([(I6, np.array([-0.9e-5, 0, 0, 0, 0, 0]), 1.0)], [0.5])),
        dict(base, name="theta-above", rot_eps=1e-9, trans_eps=1e-9, max_iters=1, make=lambda: R.scripted([(I6, np.array([-1.1e-5, 0, 0, 0, 0, 0]), 1.0)], [0.5])),
    ]
    return out


@pytest.fixture(scope="module")
def runs():
    L = load_library()
    out = []
    for case in random_cases() + designed_cases():
        ref = reference(case)
        out.append(dict(case=case, ref=ref, got=drive(L, case), ok=ref["margin"] > MARGIN_MIN))
    return out


def test_lm_state_machine_takes_the_references_decisions_and_poses(runs):
    bad = [r["case"]["name"] for r in runs if not r["ok"]]
    print(f"disqualified by a decision margin <= {MARGIN_MIN}: {len(bad)} of {len(runs)}")
    assert len(bad) <= 0.10 * len(runs), bad
    for r in runs:
        if not r["ok"]:
            continue
        got, ref, name = r["got"], r["ref"], r["case"]["name"]
        assert (got["converged"], got["outer"], got["n_err"]) == (ref["converged"], ref["outer"], ref["n_err"]), (name, got["outer"], ref["outer"], ref["census"])
        assert len(got["trials"]) == len(ref["trials"]), name
        for a, b in zip(got["trials"] + [got["pose"]], ref["trials"] + [ref["pose"]]):
            tol = LM_FACTOR * ref["cond"] * EPS * max(1.0, float(np.max(np.abs(b))))
            assert np.max(np.abs(a - b)) <= tol, (name, np.max(np.abs(a - b)), tol)


def test_lm_census(runs):
    cen = collections.Counter()
    for r in runs:
        if r["ok"]:
            cen.update(r["ref"]["census"])
    print(dict(cen))
    for lab in R.LABELS:
        assert cen[lab] >= 1, (lab, cen)


def _run(runs, name):
    return [r for r in runs if r["case"]["name"] == name][0]


def test_lm_designed_cases(runs):
    for name in ("max-iters-zero", "max-iters-negative"):
        r = _run(runs, name)
        assert (r["got"]["converged"], r["got"]["outer"], r["got"]["n_err"]) == (False, 0, 0) and r["ref"]["census"]["no_iterations"] == 1
        np.testing.assert_array_equal(r["got"]["pose"], r["case"]["guess"])
    r = _run(runs, "converged-on-rejected")
    assert r["ref"]["census"]["converged_on_rejected"] == 1 and (r["got"]["converged"], r["got"]["outer"], r["got"]["n_err"]) == (True, 1, 1)
    np.testing.assert_array_equal(r["got"]["pose"], r["case"]["guess"])
    r = _run(runs, "inner-exhausted")
    assert r["ref"]["census"]["inner_exhausted"] == 1 and r["ref"]["census"]["rejected_lambda_grown"] == 3
    assert (r["got"]["converged"], r["got"]["outer"], r["got"]["n_err"]) == (False, 1, 3)
    # the three trials were solved with lambda = 1e-9, 2e-9, 8e-9: d = -b / (1 + lambda)
    for T, lam in zip(r["got"]["trials"], (1e-9, 2e-9, 8e-9)):
        np.testing.assert_allclose(T[:3, 3] - r["case"]["guess"][:3, 3], R.quat_to_matrix(R.so3_exp(np.full(3, -0.1 / (1 + lam)))) @ r["case"]["guess"][:3, 3]
                                   - r["case"]["guess"][:3, 3] - 0.1 / (1 + lam), rtol=0, atol=1e-15)
    r = _run(runs, "rho-nan")      # NaN is neither rejected nor "accepted in the usual sense": the reference accepts it
    assert r["ref"]["census"]["rho_nan"] == 1 and r["ref"]["census"]["accepted"] == 1 and (r["got"]["converged"], r["got"]["outer"]) == (True, 1)
    r = _run(runs, "lambda-zero")
    assert r["ref"]["census"]["lambda_zero"] == 1 and (r["got"]["converged"], r["got"]["outer"], r["got"]["n_err"]) == (True, 1, 1)
    assert _run(runs, "theta-below")["ref"]["census"]["small_angle"] == 1 and _run(runs, "theta-above")["ref"]["census"]["large_angle"] == 1
    for name in ("theta-below", "theta-above"):      # the two series agree to ~theta^6: the pose is exact either side
        r = _run(runs, name)
        np.testing.assert_allclose(r["got"]["pose"], r["ref"]["pose"], rtol=0, atol=4 * EPS)
