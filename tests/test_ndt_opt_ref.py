"""csrc/ndt_opt.h on the host (pcr_ndt_opt_*, no GPU) against tests/ndt_opt_ref.py, the reference's computeTransformation /
computeStepLengthMT loop written forwards: the same objective callback drives both, and the state machine must take the reference's
decisions branch by branch.

Cases (tests/ndt_opt_cases.py): 1 032 random ones -- a 6-D quadratic of known condition number (10, 100, 1e3) with a cosine ripple of two
strengths, the fed Hessian scaled by 1, 0.2, 5 and -1, step_size 0.1, 5 and 10, trans_eps 0.01 -- plus designed ones.  A case qualifies
if the reference's smallest decision margin exceeds 1e-6 (ndt_opt_cases.MARGIN_MIN); at most 10 % may fail that.

Branch census.  Every label of ndt_opt_ref.LABELS must be seen in a qualifying case except ONE, which the reference cannot reach:

  tv3_cubic (trialValueSelectionMT case 3 choosing the cubic a_c).  Inside computeStepLengthMT's loop trialValueSelectionMT is called with the
  trial that updateIntervalMT has just seen.  After U1 (f_t > f_l) it is case 1.  After U2 or U3 a_l IS that trial (a_l = a_t, f_l = f_t,
  g_l = g_t): f_t > f_l fails, g_t * g_l = g_t^2 >= 0 fails case 2, |g_t| <= |g_l| holds: case 3 -- with a_t - a_l = 0, so z = 0 / 0 and
  a_c, a_s are NaN, `|a_c - a_t| < |a_s - a_t|` is false and the "secant" is taken, `a_t > a_l` is false, and std::max(lim, NaN) returns lim =
  a_t + 0.66 * (a_u - a_t).  So in the loop case 3 never has a finite a_c.  The one call before the loop (first trial point, a_l = 0,
  f_l = 0, g_l = (1 - mu) phi'(0) < 0) is reached only if the Wolfe test failed: either psi_t > 0 (case 1), or psi_t <= 0 and
  phi'_t > 0.9 |phi'(0)| > 0, which makes g_t * g_l < 0 (case 2), or psi_t is NaN -- then z and a_c are NaN again.  Case 3 with
  a_t > a_l (tv3_min) and case 4 (tv4) are reachable by that last door only: a NaN score at the first trial point, the slope choosing
  between them (designed cases score-nan-case3-min and score-nan-case4).

The labels the random families reach on their own must each be seen at least 10 times (SIMPLE_LABELS)."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

import ndt_opt_cases as K
import ndt_opt_ref as R
from simpleslam_amd.pcr import load_library

UNREACHABLE = ("tv3_cubic",)
SIMPLE_LABELS = ("tv1_cubic", "tv1_average", "tv2_cubic", "tv2_secant", "tv3_secant", "tv3_max", "ui_u1", "ui_u2", "ui_u3", "ui_converged",
                 "interval_closed", "trial_on_closed", "end_cap", "end_interval_converged", "end_wolfe_first", "end_wolfe_later",
                 "dir_flipped", "clamp_high", "clamp_low", "trial_repeat")


@pytest.fixture(scope="module")
def runs():
    """every case once: the reference, the state machine as it runs by default and with repeats evaluated"""
    L = load_library()
    out = []
    for case in K.base_cases() + K.designed_cases():
        got = K.drive(L, case)
        ref = K.reference(case, got["p0"])
        # (p0 = the guess's Euler angles as Eigen's eulerAngles(0, 1, 2) extracts them, in float: another triple of the same rotation)
        assert np.max(np.abs(R.float_pose(got["p0"]).astype(np.float64) - R.float_pose(case["p_init"]))) < 2e-6, case["name"]
        out.append(dict(case=case, ref=ref, got=got, got_off=K.drive(L, case, replay_off=True), ok=ref["margin"] > K.MARGIN_MIN))
    return out


def test_most_cases_qualify(runs):
    bad = [r["case"]["name"] for r in runs if not r["ok"]]
    share = len(bad) / len(runs)
    print(f"disqualified by a decision margin <= {K.MARGIN_MIN}: {len(bad)} of {len(runs)} cases = {100 * share:.1f} %")
    assert share <= 0.10
    assert all(r["ok"] for r in runs if r["case"]["family"] == "designed"), bad


def test_state_machine_takes_the_references_decisions(runs):
    for r in runs:
        if r["ok"]:
            K.check_against_reference(r["got"], r["ref"], r["case"], replay_off=False)
            K.check_against_reference(r["got_off"], r["ref"], r["case"], replay_off=True)


def test_replayed_and_evaluated_repeats_decide_alike_bit_for_bit(runs):
    """ctl_replay_run (the repeats answered on local copies) against ctl_advance (every repeat a fed evaluation): the same decisions,
    the same points and the same final pose to the bit -- for EVERY case, qualifying or not: both runs use the same solve."""
    seen = collections.Counter()
    for r in runs:
        a, b, name = r["got"], r["got_off"], r["case"]["name"]
        assert (a["converged"], a["iterations"], a["evaluations"], a["hessians"]) == (b["converged"], b["iterations"], b["evaluations"], b["hessians"]), name
        pa = [p.tobytes() for p, _ in K.distinct_points([(k, p) for k, p, _ in a["requests"]])]
        pb = [p.tobytes() for p, _ in K.distinct_points([(k, p) for k, p, _ in b["requests"]])]
        assert pa == pb, name
        assert a["pose"].tobytes() == b["pose"].tobytes() and (a["a_t"] == b["a_t"] or (a["a_t"] != a["a_t"] and b["a_t"] != b["a_t"])), name
        assert sum(1 for k, _, _ in b["requests"] if k != "h") == b["evaluations"], name
        if a["replayed"]:
            for lab in R.REPEAT_LABELS:
                seen[lab] += r["ref"]["census"][lab]
    # the replay runs pass through the closing of the interval, end by the cap and end by update_interval's "converged"
    assert seen["repeat_closes_interval"] >= 1 and seen["repeat_ends_by_cap"] >= 10 and seen["repeat_ends_by_ui_converged"] >= 1, seen


def test_census_covers_every_reachable_branch(runs):
    cen = collections.Counter()
    for r in runs:
        if r["ok"]:
            cen.update(r["ref"]["census"])
    print({lab: cen[lab] for lab in R.LABELS + R.REPEAT_LABELS})
    assert len(UNREACHABLE) <= 3 and not set(UNREACHABLE) & set(SIMPLE_LABELS)
    for lab in R.LABELS:
        if lab in UNREACHABLE:
            assert cen[lab] == 0, lab      # (the argument in this module's docstring says never: a count would refute it)
        else:
            assert cen[lab] >= (10 if lab in SIMPLE_LABELS else 1), (lab, cen[lab])


def _run(runs, name):
    return [r for r in runs if r["case"]["name"] == name][0]


def test_designed_degenerate_steps(runs):
    r = _run(runs, "dphi0-zero")      # step 0 twice: nr_iterations 0 does not converge, nr_iterations 1 does; the pose stays the guess
    assert r["ref"]["census"]["dphi0_zero"] == 2 and (r["got"]["converged"], r["got"]["iterations"], r["got"]["evaluations"]) == (True, 2, 1)
    assert r["ref"]["steps"] == [0.0, 0.0]
    np.testing.assert_array_equal(r["got"]["pose"], R.float_pose(r["case"]["p_init"]))
    r = _run(runs, "nrm-zero")
    assert r["ref"]["census"]["nrm_zero"] == 1 and (r["got"]["converged"], r["got"]["iterations"], len(r["got"]["requests"])) == (True, 0, 1)
    r = _run(runs, "grad-nan")
    assert r["ref"]["census"]["nrm_nan"] == 1 and (r["got"]["converged"], r["got"]["iterations"], len(r["got"]["requests"])) == (False, 0, 1)


def test_nan_score_inside_a_search(runs):
    """std::min(a_t, step_max) and std::max(a_t, step_min) return their first argument unless the comparison holds: a NaN trial stays NaN"""
    assert math.isnan(R.std_min(math.nan, 1.0)) and R.std_min(1.0, math.nan) == 1.0
    assert math.isnan(R.std_max(math.nan, 1.0)) and R.std_max(1.0, math.nan) == 1.0
    r = _run(runs, "score-nan-case4")
    assert r["ref"]["census"]["tv4"] == 1
    for run in (r["got"], r["got_off"]):
        assert np.all(np.isnan(run["requests"][2][1])) and run["requests"][2][0] == "d"      # guess, first trial, then the NaN point
    r = _run(runs, "score-nan-case3-min")
    assert r["ref"]["census"]["tv3_min"] == 1 and r["ref"]["census"]["tv3_secant"] >= 1
    # a_l = 0, a_t = 1, g_l = (1 - 1e-4) * -2, g_t = -1 + 2e-4: the secant a_s = g_l / (g_l - g_t) = 2 exceeds lim = 0.34: the third point is at 0.34
    p0, p2 = r["got"]["requests"][0][1], r["got"]["requests"][2][1]
    np.testing.assert_allclose(p2 - p0, [0.34, 0, 0, 0, 0, 0], rtol=0, atol=1e-15)


def test_loop_ends(runs):
    for mi, its in ((0, 2), (1, 3)):      # nr_iterations > max_iterations is tested BEFORE the increment: max_iters + 2 Newton steps
        r = _run(runs, f"max-iters-{mi}")
        assert (r["got"]["iterations"], r["got"]["converged"]) == (its, True) and r["ref"]["iterations"] == its
    r = _run(runs, "starts-converged-0")     # every step is step_min = trans_eps / 2 < trans_eps: converged after the second
    assert r["ref"]["census"]["end_interval_converged"] == 2 and r["ref"]["steps"] == [0.005, 0.005] and r["got"]["iterations"] == 2
    assert r["got"]["hessians"] == 0 and r["got"]["evaluations"] == 3


def test_host_pose_and_tables_are_the_references_to_the_bit(runs):
    """Every requested pose is Translation * Rx * Ry * Rz in float with the C library's sinf / cosf (the check on glibc_sincosf), and the
    angle tables are computeAngleDerivatives' -- including the float entry that has sy where the double table has -sy.  On the host both
    sides call the same libm: equal bits."""
    L = load_library()
    checked = [0]

    def on_request(o, i, req):
        kind, p6, pose = req
        if i == 0:
            return      # (the guess's pose is the caller's matrix, not a product)
        np.testing.assert_array_equal(pose, R.float_pose(p6))
        j, h, jd, hd = np.zeros((8, 3), np.float32), np.zeros((15, 3), np.float32), np.zeros((8, 3)), np.zeros((15, 3))
        assert L.pcr_ndt_opt_tables(o, j.ctypes.data_as(K.FP), h.ctypes.data_as(K.FP), jd.ctypes.data_as(K.DP), hd.ctypes.data_as(K.DP)) == 0
        rj, rh, rjd, rhd = R.angle_tables(p6)
        for a, b in ((j, rj), (h, rh), (jd, rjd), (hd, rhd)):
            np.testing.assert_array_equal(a, b)
        assert h[6, 2] == np.float32(-hd[6, 2]) and (hd[6, 2] != 0 or i == 0)
        checked[0] += 1
    for r in runs[:60:5] + [_run(runs, "quartic-overshoot"), _run(runs, "small-angles")]:
        K.drive(L, r["case"], on_request=on_request)
    assert checked[0] > 100


def test_calls_on_a_null_object_fail():
    L = load_library()
    k = C.c_int(0)
    assert L.pcr_ndt_opt_request(None, C.byref(k), None, None) == 1 and L.pcr_ndt_opt_feed(None, np.zeros(43).ctypes.data_as(K.DP)) == 1
    assert L.pcr_ndt_opt_set_replay(None, 1) == 1 and L.pcr_ndt_opt_state(None, None, None, None, None) == 1
