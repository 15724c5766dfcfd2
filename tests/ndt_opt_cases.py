"""The cases tests/test_ndt_opt_ref.py (host) and tests/test_ndt_opt_gpu.py (device) run through the NDT state machine, and the driver
that feeds a pcr_ndt_opt object from an objective callback of tests/ndt_opt_ref.py.

A case is dict(name, make -> callback, p_init, step_size, trans_eps, max_iters, cond).  Callbacks may keep state (scripted), so every run
gets a fresh one from make()."""
import ctypes as C
import math

import numpy as np

import ndt_opt_ref as R

DP = C.POINTER(C.c_double)
FP = C.POINTER(C.c_float)
KIND = {0: "dh", 1: "d", 2: "h"}

# A qualifying case's smallest decision margin (ndt_opt_ref: relative distance of the two sides of a comparison) must exceed this: two
# 6x6 solves of a matrix with cond <= 1e3 differ by ~1e3 * eps = 2e-13 of the step, seven orders below it.
MARGIN_MIN = 1e-6
# |p_library - p_reference| <= P_FACTOR * cond(H) * eps * scale for every requested point, scale = max(1, |p|_inf, the longest step
# a_t = |x_t - x| taken so far in the run): the error of a direction reaches a point multiplied by the step actually taken along it, and
# the errors of earlier steps stay in p.  Each Newton direction carries the forward error of a backward-stable 6x6 solve,
# c * cond * eps with c ~ n^2 = 36 for either SVD and for the pivoted elimination; a run is at most 36 Newton iterations whose errors
# add (the searches of the qualifying cases are contractions or clamped steps): 36 * 36 = 1296, rounded down to 1e3 since the errors of
# the iterations do not all align.
P_FACTOR = 1e3


def p_tolerance(cond, p, longest_step):
    fin = np.abs(p[np.isfinite(p)])
    return P_FACTOR * cond * R.EPS * max(1.0, float(longest_step), float(np.max(fin)) if fin.size else 0.0)


def pose16(T):
    """4x4 (float) -> the column-major 16 doubles the C ABI takes"""
    return np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16).copy()


def drive(L, case, replay_off=False, device=False, on_request=None, after_feed=None, limit=3000):
    """Runs `case` through a pcr_ndt_opt (host, or pcr_ndt_opt_create_device).  -> dict(requests [(kind, p6, pose 4x4 float32)], p0,
    converged, iterations, evaluations, hessians, replayed, late_h, bail, pose)"""
    f = case["make"]()
    guess = pose16(R.float_pose(case["p_init"]))
    create = L.pcr_ndt_opt_create_device if device else L.pcr_ndt_opt_create
    o = create(guess.ctypes.data_as(DP), float(case["step_size"]), float(case["trans_eps"]), int(case["max_iters"]))
    assert o, "no optimiser object"
    try:
        if replay_off:
            assert L.pcr_ndt_opt_set_replay(o, 1) == 0
        reqs = []
        for _ in range(limit):
            kind, p6, pose = C.c_int(-1), np.zeros(6), np.zeros(16)
            assert L.pcr_ndt_opt_request(o, C.byref(kind), p6.ctypes.data_as(DP), pose.ctypes.data_as(DP)) == 0
            if kind.value == 3:
                break
            reqs.append((KIND[kind.value], p6.copy(), pose.reshape(4, 4).T.astype(np.float32)))
            if on_request is not None:
                on_request(o, len(reqs) - 1, reqs[-1])
            score, grad, hess = f(p6.copy(), KIND[kind.value])
            sums = np.zeros(43)
            sums[0] = score; sums[1:7] = grad; sums[7:] = np.asarray(hess).reshape(36)
            if kind.value == 1:
                sums[7:] = case.get("light_sentinel", 0.0)      # a pass without the Hessian delivers nothing there: must be ignored
            assert L.pcr_ndt_opt_feed(o, sums.ctypes.data_as(DP)) == 0
            if after_feed is not None:
                after_feed(o, reqs[-1], sums)
        else:
            raise AssertionError("the optimiser did not finish")
        pose, conv, its, done = np.zeros(16), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.pcr_ndt_opt_result(o, pose.ctypes.data_as(DP), C.byref(conv), C.byref(its), C.byref(done)) == 0 and done.value == 1
        ev, hs, rep = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.pcr_ndt_opt_counts(o, C.byref(ev), C.byref(hs), C.byref(rep)) == 0
        bail, late, a_t, phase = C.c_int(0), C.c_int(0), C.c_double(0), C.c_int(0)
        assert L.pcr_ndt_opt_state(o, C.byref(bail), C.byref(late), C.byref(a_t), C.byref(phase)) == 0
        # after done: a request says "none", a feed is refused
        kind = C.c_int(-1)
        assert L.pcr_ndt_opt_request(o, C.byref(kind), None, None) == 0 and kind.value == 3
        assert L.pcr_ndt_opt_feed(o, np.zeros(43).ctypes.data_as(DP)) == 1
        return dict(requests=reqs, p0=reqs[0][1] if reqs else None, converged=bool(conv.value), iterations=its.value, evaluations=ev.value,
                    hessians=hs.value, replayed=rep.value, late_h=late.value, bail=bail.value, a_t=a_t.value,
                    pose=pose.reshape(4, 4).T.astype(np.float32))
    finally:
        L.pcr_ndt_opt_destroy(o)


def reference(case, p0):
    return R.align(case["make"](), p0, case["step_size"], case["trans_eps"], case["max_iters"], T0=R.float_pose(case["p_init"]))


def distinct_points(log):
    """An evaluation log as the sequence of points it visits and what was evaluated there: repeats of a point the machine answers itself
    and the late Hessian at a first trial point fold into the point's entry.  -> [(p6, "d" or "dh..", has computeHessian)]"""
    out = []
    for kind, p in log:
        if out and np.array_equal(out[-1][0], p, equal_nan=True):
            if kind == "h":
                out[-1][1] = True
            continue
        assert kind != "h", "a computeHessian at a point nothing was evaluated at"
        out.append([p, False])
    return out


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def check_against_reference(got, ref, case, replay_off):
    """the assertions of one run against the reference's (see tests/test_ndt_opt_ref.py)"""
    name = case["name"]
    assert got["bail"] == 0, name
    assert (got["converged"], got["iterations"], got["evaluations"], got["hessians"]) == \
           (ref["converged"], ref["iterations"], ref["n_deriv"], ref["n_hess"]), (name, got, ref["census"])
    lib_log = [(k, p) for k, p, _ in got["requests"]]
    if replay_off:      # the reference's own schedule: every evaluation, kind by kind
        assert [k for k, _ in lib_log] == [k for k, _ in ref["log"]], name
        assert got["replayed"] == 0 and got["late_h"] == 0, name
    else:               # evaluations = requests that are not late Hessians + repeats answered without asking
        n_late = sum(1 for i, (k, p) in enumerate(lib_log) if k == "dh" and i > 0)
        assert n_late == got["late_h"], name
        assert got["evaluations"] == sum(1 for k, _ in lib_log if k != "h") - n_late + got["replayed"], name
        for i, (k, p) in enumerate(lib_log):
            if k == "dh" and i > 0:
                assert lib_log[i - 1][0] == "d" and np.array_equal(lib_log[i - 1][1], p), name
    a, b = distinct_points(lib_log), distinct_points(ref["log"])
    assert len(a) == len(b), (name, len(a), len(b))
    steps = {}      # the step from its search's start to every point of the reference's log
    for (_, p), x in zip(ref["log"], ref["log_x"]):
        d = p - x
        steps[p.tobytes()] = float(np.sqrt(np.sum(d[np.isfinite(d)] ** 2)))
    longest = 0.0
    for (pa, ha), (pb, hb) in zip(a, b):
        assert ha == hb, name
        assert same_nan(pa, pb), name
        fin = np.isfinite(pb)
        longest = max(longest, steps[pb.tobytes()])
        tol = p_tolerance(case["cond"], pb, longest)
        assert np.all(np.abs(pa[fin] - pb[fin]) <= tol), (name, pa, pb, tol)
    # the final pose as Matrix4f: float roundings of p (differing by at most p_tolerance) through <= 4 chained float operations per entry: 4 ulp
    tol = 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(ref["pose"].astype(np.float64)))
    assert same_nan(got["pose"], ref["pose"]), name
    fin = np.isfinite(ref["pose"])
    assert np.all(np.abs(got["pose"].astype(np.float64) - ref["pose"])[fin] <= tol[fin]), (name, got["pose"], ref["pose"])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _quadratic_case(family, seed, hess_scale, step_size, max_iters=12):
    rng = np.random.default_rng(1000 * seed + 7)
    cond = float((10.0, 100.0, 1000.0)[seed % 3])
    A = R.spd_with_condition(rng, cond)
    c = np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, 0.3, 3)])
    p_init = c + np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 0.15, 3)]) * (4.0 if seed % 2 else 1.0)
    ripple, fscale = FAMILIES[family]
    freq = rng.normal(0, fscale, (3, 6))
    return dict(name=f"{family}-s{seed}-h{hess_scale}-st{step_size}", family=family, cond=cond, p_init=p_init, step_size=step_size, trans_eps=0.01,
                max_iters=max_iters, make=lambda: R.quadratic(A, c, hess_scale, ripple, freq))


# amplitude of the cosine ripple on the quadratic and the spread of its three wave vectors.  (No pure quadratic: along a line its cubic and
# quadratic interpolants coincide, so trial_value's case 1 compares two equal numbers up to rounding, and every such run is disqualified.)
FAMILIES = {"mild": (0.02, 3.5), "ripple": (0.03, 4.0)}


def base_cases(seeds=range(43)):
    out = []
    for family in FAMILIES:
        for seed in seeds:
            for hs in (1.0, 0.2, 5.0, -1.0):
                for st in (0.1, 5.0, 10.0):
                    out.append(_quadratic_case(family, seed, hs, st))
    return out


def _scripted_case(name, entries, p_init=(0.25, -0.5, 1.0, 0.05, -0.1, 0.2), step_size=1.0, trans_eps=0.01, max_iters=3, cond=1.0):
    return dict(name=name, family="designed", cond=cond, p_init=np.array(p_init, np.float64), step_size=step_size, trans_eps=trans_eps,
                max_iters=max_iters, make=lambda: R.scripted(entries))


def designed_cases():
    I6 = np.eye(6).reshape(36)
    nan = math.nan
    out = []
    # d_phi_0 == 0: the Newton step of H = diag(1, -1, 1, ..) is orthogonal to the gradient (1, 1, 0, ..): step 0, twice, converged
    out.append(_scripted_case("dphi0-zero", [(-1.0, (1, 1, 0, 0, 0, 0), np.diag([1.0, -1, 1, 1, 1, 1]))]))
    out.append(_scripted_case("nrm-zero", [(-1.0, np.zeros(6), -I6)]))
    out.append(_scripted_case("grad-nan", [(-1.0, (0.5, nan, 0, 0, 0, 0), -I6)]))
    # A NaN score at the first trial point.  phi(0) = 1, gradient 2 along -x: the Newton step of H = -I is (−2, 0, ..), clamped to 1.
    # NaN fails f_t > f_l and the Wolfe test; with g_t of the sign of g_l the slope alone picks the case:
    #   |g_t| > |g_l|  -> case 4, whose cubic through a NaN value is NaN; std::min(NaN, step_max) and std::max(NaN, step_min) keep the NaN
    #                     (both return their FIRST argument unless the comparison holds): the next point is all NaN
    #   |g_t| <= |g_l| -> case 3 with a_t > a_l: a_c is NaN, the secant a_s is not; std::min(lim, a_s)
    g0 = (2.0, 0, 0, 0, 0, 0)
    tail = [(-0.5, (0.1, 0, 0, 0, 0, 0), -I6)]
    out.append(_scripted_case("score-nan-case4", [(-1.0, g0, -I6), (nan, (3.0, 0, 0, 0, 0, 0), -I6)] + tail, max_iters=1))
    out.append(_scripted_case("score-nan-case3-min", [(-1.0, g0, -I6), (nan, (1.0, 0, 0, 0, 0, 0), -I6)] + tail, max_iters=1))
    # the loop's ends
    rng = np.random.default_rng(5)
    A = R.spd_with_condition(rng, 10.0)
    c = np.array([0.5, 0.2, -0.3, 0.1, 0.05, -0.2])
    for mi in (0, 1):
        out.append(dict(name=f"max-iters-{mi}", family="designed", cond=10.0, p_init=c + 0.7, step_size=0.1, trans_eps=0.01, max_iters=mi,
                        make=lambda: R.quadratic(A, c)))
    # step_size < trans_eps / 2: the interval starts converged, every step is step_min
    for k in range(8):
        out.append(dict(name=f"starts-converged-{k}", family="designed", cond=10.0, p_init=c + 0.7 - 0.1 * k, step_size=0.004 - 0.0004 * k, trans_eps=0.01,
                        max_iters=4, make=lambda: R.quadratic(A, c)))
    # A repeat that closes the interval: the Newton step (0.002) is below step_min (0.005) and clamped up to it; there the value has
    # dropped (psi < 0) and the slope has turned steeply positive, so the search goes on (case 2), wants a shorter step and is clamped to
    # step_min again: the SAME point, whose second look closes the interval (the first evaluation of a search is never tested for that),
    # updates it (U3), asks for 0.34 * a_t (case 3 with a_t == a_l: a_c and a_s are NaN), is clamped once more, and the third look
    # finds g_t * (a_l - a_t) == 0: "interval converged".
    for k in range(8):
        out.append(_scripted_case(f"repeat-closes-interval-{k}", [(-1.0, (0.002 + 0.0003 * k, 0, 0, 0, 0, 0), -I6),
                                                                   (-0.999999, (-0.01 * (k + 1), 0, 0, 0, 0, 0), -I6)], max_iters=1))
    # 1-D profiles (the other five directions stiff).  A quartic whose Newton step overshoots the minimum; -cos started beyond its inflection
    # (max_iters 1: the far-slope searches only -- near the minimum -cos is a quadratic, whose case-1 comparison is a tie up to rounding)
    u = np.array([1.0, 2.0, -1.0, 0.5, 0.25, -0.5])
    base = np.array([0.1, 0.2, 0.3, 0.02, -0.03, 0.04])
    un = u / np.linalg.norm(u)
    out.append(dict(name="quartic-overshoot", family="designed", cond=50.0, p_init=base - 1.0 * un, step_size=5.0, trans_eps=0.01, max_iters=6,
                    make=lambda: R.profile_1d(u, base, lambda a: 0.25 * a ** 4 + 0.5 * a * a, lambda a: a ** 3 + a, lambda a: 0.3)))
    out.append(dict(name="cos-far-slope", family="designed", cond=50.0, p_init=base - 2.0 * un, step_size=5.0, trans_eps=0.01, max_iters=1,
                    make=lambda: R.profile_1d(u, base, lambda a: -math.cos(a), lambda a: math.sin(a), lambda a: 0.25)))
    # computeAngleDerivatives' small-angle shortcut (|angle| < 10e-5: sine 0, cosine 1) on both sides: angles of 0.5e-4, 2e-4 and -0.5e-4
    # that stay where they are while the steps go along x
    out.append(_scripted_case("small-angles", [(-1.0, (0.3, 0, 0, 0, 0, 0), -I6), (-0.9, (0.03, 0, 0, 0, 0, 0), -I6), (-0.89, (0.001, 0, 0, 0, 0, 0), -I6)],
                              p_init=(0.25, -0.5, 1.0, 0.5e-4, 2e-4, -0.5e-4), max_iters=3))
    return out
