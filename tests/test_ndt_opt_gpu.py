"""The NDT controller step as the DEVICE runs it -- ndt_ctl_kernel: ndt_ctl_step_block over five waves, the guarded elimination instead of
the SVD, the device's libm, glibc_sincosf with the device's fma -- stepped one feed at a time through pcr_ndt_opt_create_device and held
against tests/ndt_opt_ref.py, the reference's loop written forwards, and against a host object fed the same callback."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

import ndt_opt_cases as K
import ndt_opt_ref as R
from simpleslam_amd.pcr import load_library

pytestmark = pytest.mark.gpu

# Double tables: every entry is a sum of at most two products of at most three sines / cosines.  The device's double sin / cos are within
# 2 ulp (HIP's documented bound), every factor is <= 1 in magnitude: a product of three carries 3 * 2 ulp + 2 roundings of half an ulp = 7 ulp
# of 1, a sum of two 14.5 ulp, the reference's own evaluation (correctly rounded factors) 2 * (1.5 + 1) + 0.5 = 5.5 ulp: 20 ulp of 1 = 20 * 2^-53.
TABLE_TOL = 20 * 2.0 ** -53


def _tables(L, o):
    j, h, jd, hd = np.zeros((8, 3), np.float32), np.zeros((15, 3), np.float32), np.zeros((8, 3)), np.zeros((15, 3))
    assert L.pcr_ndt_opt_tables(o, j.ctypes.data_as(K.FP), h.ctypes.data_as(K.FP), jd.ctypes.data_as(K.DP), hd.ctypes.data_as(K.DP)) == 0
    return j, h, jd, hd


@pytest.fixture(scope="module")
def chosen(gpu):
    """about 60 qualifying cases that together show every reachable census label: the designed ones, then random ones picked greedily"""
    L = load_library()
    picked, cen = [], collections.Counter()
    cases = K.designed_cases() + K.base_cases(range(12))
    for case in cases:
        got = K.drive(L, case)
        ref = K.reference(case, got["p0"])
        if not ref["margin"] > K.MARGIN_MIN:
            continue
        new = [lab for lab in ref["census"] if cen[lab] < 3]
        if case["family"] == "designed" or (new and len(picked) < 64):
            picked.append(dict(case=case, ref=ref, host=got))
            cen.update(ref["census"])
    assert all(cen[lab] for lab in R.LABELS if lab != "tv3_cubic"), cen
    assert cen["repeat_closes_interval"] and cen["repeat_ends_by_cap"] and cen["repeat_ends_by_ui_converged"]
    return L, picked


def test_device_steps_take_the_references_and_the_hosts_decisions(chosen):
    L, picked = chosen
    moved_entries = np.zeros(69, bool)
    small = [False]      # a point with angles on both sides of computeAngleDerivatives' 10e-5 shortcut was visited (case small-angles)
    for r in picked:
        case, ref, host = r["case"], r["ref"], r["host"]
        prev = {}

        def on_request(o, i, req):
            kind, p6, pose = req
            if i == 0 or not np.all(np.isfinite(p6)):
                return
            if prev.get("p") is not None and np.array_equal(prev["p"], p6):
                return
            # the float pose: Translation * Rx * Ry * Rz with the C library's sinf / cosf, to the bit
            np.testing.assert_array_equal(pose, R.float_pose(p6), err_msg=case["name"])
            j, h, jd, hd = _tables(L, o)
            rj, rh, rjd, rhd = R.angle_tables(p6)
            assert np.max(np.abs(jd - rjd)) <= TABLE_TOL and np.max(np.abs(hd - rhd)) <= TABLE_TOL, case["name"]
            hf = hd.astype(np.float32); hf[6, 2] = -hf[6, 2]      # the float table has sy where the double one has -sy
            np.testing.assert_array_equal(j, jd.astype(np.float32)); np.testing.assert_array_equal(h, hf)
            # every one of the 69 entries is written by this step: wherever the reference's table moved since the previous step (by more
            # than rounding), the device's must differ from the previous step's device table -- a part left out by a wave is a stale row
            dev_t = np.concatenate([jd.ravel(), hd.ravel()]); ref_t = np.concatenate([rjd.ravel(), rhd.ravel()])
            if prev.get("t") is not None:
                moved = np.abs(ref_t - prev["t"]) > 4 * TABLE_TOL
                assert np.all(dev_t[moved] != prev["dev"][moved]), (case["name"], np.nonzero(moved & (dev_t == prev["dev"]))[0])
                moved_entries[:] |= moved
            prev["t"] = ref_t; prev["dev"] = dev_t; prev["p"] = p6.copy()
            small[0] |= bool(np.any(np.abs(p6[3:]) < 10e-5) and np.any((np.abs(p6[3:]) > 10e-5) & (np.abs(p6[3:]) < 3e-4)))
        dev = K.drive(L, case, device=True, on_request=on_request)
        if case["name"] == "grad-nan":      # a gradient that is not finite: the guarded solve hands the call to the host, which finds the NaN norm
            assert (dev["bail"], len(dev["requests"]), dev["converged"], dev["iterations"]) == (1, 1, False, 0)
            continue
        K.check_against_reference(dev, ref, case, replay_off=False)
        assert [k for k, _, _ in dev["requests"]] == [k for k, _, _ in host["requests"]], case["name"]
        assert (dev["converged"], dev["iterations"], dev["evaluations"], dev["hessians"], dev["replayed"], dev["late_h"]) == \
               (host["converged"], host["iterations"], host["evaluations"], host["hessians"], host["replayed"], host["late_h"]), case["name"]
    zeros = np.concatenate([R.angle_tables(np.full(6, 0.3))[2].ravel(), R.angle_tables(np.full(6, 0.3))[3].ravel()]) == 0
    assert small[0]
    assert np.all(moved_entries | zeros) and zeros.sum() == 11      # (the constant zeros of j_ang_f_.. and h_ang_c2_..)


def test_device_replay_matches_evaluated_repeats(chosen):
    L, picked = chosen
    n = 0
    for r in picked:
        if not r["host"]["replayed"]:
            continue
        dev = K.drive(L, r["case"], device=True, replay_off=True)
        K.check_against_reference(dev, r["ref"], r["case"], replay_off=True)
        n += 1
    assert n >= 5


def _hess_case(name, H, cond, step_size):
    g = (0.3, -0.2, 0.1, 0.05, -0.04, 0.02)
    I6 = np.eye(6)
    return K._scripted_case(name, [(-1.0, g, -np.asarray(H, np.float64)), (-0.9, tuple(0.1 * v for v in g), -I6), (-0.89, tuple(0.01 * v for v in g), -I6)],
                            step_size=step_size, max_iters=2, cond=cond)


def test_guarded_pivot_hands_the_call_back(gpu):
    """lu6_solve_guarded gives up when a pivot is not above 1e-9 of the largest entry, or anything is not finite: the device object ends
    with bail = 1, done, kind "none" on that feed; the host's SVD goes on with the pseudo-inverse, as the reference does.  Just above the
    guard the device's step agrees with the reference's within P_FACTOR * cond * eps of the step taken (ndt_opt_cases.p_tolerance: the
    weak direction is x, its step 0.3 / 2e-9 = 1.5e8, left unclamped by step_size = 1e9 in that pair of cases alone; cond = 1 / 2e-9)."""
    L = load_library()
    def weak(v):
        return np.diag([v, 1, 1, 1, 1, 1.0])
    inf = np.eye(6); inf[2, 2] = math.inf
    for name, H, cond, step_size, bails in (("rank5", weak(0.0), 1.0, 1.0, True), ("zero", np.zeros((6, 6)), 1.0, 1.0, True), ("inf", inf, 1.0, 1.0, True),
                                            ("below", weak(0.5e-9), 2e9, 1e9, True), ("above", weak(2e-9), 0.5e9, 1e9, False)):
        case = _hess_case(name, H, cond, step_size)
        host = K.drive(L, case)
        ref = K.reference(case, host["p0"])
        K.check_against_reference(host, ref, case, replay_off=False)
        dev = K.drive(L, case, device=True)
        if bails:
            assert (dev["bail"], len(dev["requests"]), dev["converged"], dev["iterations"]) == (1, 1, False, 0), (name, dev)
        else:
            K.check_against_reference(dev, ref, case, replay_off=False)
            assert abs(dev["requests"][1][1][0] - dev["requests"][0][1][0]) > 1e8      # (the long step was taken)


def test_hessian_slots_are_taken_from_the_passes_that_deliver_them(chosen):
    """a pass with the Hessian, a computeHessian pass and a late Hessian store the 36 entries they delivered; a light pass leaves zeros
    whatever its slots 7..42 hold"""
    L, picked = chosen
    seen = collections.Counter()
    for r in picked[::4]:
        case = dict(r["case"], light_sentinel=-7.25e11)
        log = []

        def after_feed(o, req, sums):
            H = np.zeros(36)
            assert L.pcr_ndt_opt_hessian(o, H.ctypes.data_as(K.DP)) == 0
            log.append((req[0], H, sums[7:].copy()))
        dev = K.drive(L, case, device=True, after_feed=after_feed)
        K.check_against_reference(dev, r["ref"], r["case"], replay_off=False)
        for kind, H, fed in log:
            seen[kind] += 1
            if kind == "d":
                assert not np.any(H), case["name"]
            else:
                np.testing.assert_array_equal(H, fed)
    assert seen["d"] and seen["dh"] > len(picked[::4]) and seen["h"]
