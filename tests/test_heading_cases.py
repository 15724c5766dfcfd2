"""The heading cases (tests/heading_cases.py) on the CPU: every case reaches the branch it claims, the float32 Euler restatement is right,
and every case is one the five references solve from its guess -- a condition on the cases, checked before the device is asked anything."""
import numpy as np
import pytest

import heading_cases as H
from simpleslam_amd import synth


def test_the_table_is_the_issues():
    plain = [(c["yaw_deg"], c["roll"], c["pitch"]) for c in H.CASES if c["scene"] == "plain"]
    for yaw in (0, 90, -90, 119, 121, 179.9, 180, -179.9):
        assert (yaw, 0.01, -0.01) in plain and (yaw, -0.01, 0.01) in plain
    for yaw in (0, 90, 180):
        assert (yaw, 0.0, 0.0) in plain
    assert sorted(c["scene"] for c in H.CASES if c["scene"] != "plain") == ["rot_x", "rot_y"]
    assert len(H.CASES) == 21 and len(set(H.NAMES)) == 21
    c = H.case("plain-yaw0-+-")
    assert c["scan"].shape == (8192, 4) and c["map"].shape == (30_000, 4)
    world, _ = H._world()
    np.testing.assert_array_equal(c["truth"][:3, 3], synth.scan_pose(world, 0, 5)[:3, 3])
    assert [c["name"] for c in H.CASES if c["position"] != 0] == ["plain-yaw-179.9--+"]      # (the one case its references solve only further along the street)


@pytest.mark.parametrize("name", H.NAMES)
def test_case_reaches_the_branch_it_claims(name):
    c = H.case(name)
    for T in (c["truth"], c["init"]):      # one degree of perturbation must not carry the guess into another branch of t2se3
        R = T[:3, :3]
        tr = np.trace(R)
        if c["route"] == "q":
            assert tr > 0 and H.t2se3_route(R) == "q"
        else:
            assert tr <= 0 and int(np.argmax(np.diag(R))) == c["route"] == H.t2se3_route(R)
    Rf = c["truth"][:3, :3].astype(np.float32)
    r0 = np.arctan2(Rf[1, 2], Rf[2, 2])
    assert r0.dtype == np.float32
    assert {"pi": r0 > 0, "zero": r0 < 0, "edge": r0 == 0}[c["family"]], (name, r0)
    assert H.euler_family(c["truth"][:3, :3]) == c["family"]
    if c["scene"] != "plain":      # the poses turned over have a first angle next to pi without the flip
        assert abs(abs(H.euler_xyz_f32(c["truth"][:3, :3])[0]) - np.pi) < 0.02


def test_every_branch_occurs_often_enough():
    routes = [c["route"] for c in H.CASES]
    assert {0, 1, 2, "q"} <= set(routes)
    near_zero = near_pi = 0
    for c in H.CASES:
        e = H.euler_xyz_f32(H.case(c["name"])["truth"][:3, :3])
        near_zero += bool(abs(e[0]) < 0.02 and abs(e[1]) < 0.02)
        near_pi += bool(abs(abs(e[0]) - np.pi) < 0.02 and abs(abs(e[1]) - np.pi) < 0.02)
    assert near_zero >= 4 and near_pi >= 4, (near_zero, near_pi)
    assert sum(c["family"] == "pi" for c in H.CASES) >= 4 and sum(c["family"] == "zero" for c in H.CASES) >= 4
    assert sum(c["family"] == "edge" for c in H.CASES) == 3
    assert {H.BY_NAME[n]["route"] for n in H.VARIANT_CASES} == {0, 1, 2}


@pytest.mark.parametrize("name", H.NAMES)
def test_euler_xyz_f32_rebuilds_the_rotation(name):
    """oracle.ndt_scan2map does not hand out its start parameters, so: Rx(e0) Ry(e1) Rz(e2) of the angles is R again within float32's
    rounding of R -- R's entries are rounded to float (half an epsilon of entries up to 1), the three angles are each a few float ulps of pi
    off, and an angle error shows one to one in the entries: 16 epsilon covers both -- and the angles are in eulerAngles' ranges
    ([0, pi] for the first after the sign flip, [-pi, pi] for the others)."""
    for T in (H.case(name)["truth"], H.case(name)["init"]):
        R = T[:3, :3]
        e = H.euler_xyz_f32(R)
        assert e.dtype == np.float32
        assert -1e-7 <= e[0] <= np.float32(np.pi) and (np.abs(e[1:]) <= np.float32(np.pi)).all()
        assert np.abs(H.rot_xyz(e) - R).max() <= 16 * np.finfo(np.float32).eps
        p6 = H.ndt_p6(T)
        np.testing.assert_array_equal(p6[:3], T[:3, 3].astype(np.float32))
        np.testing.assert_array_equal(p6[3:], e)


def test_euler_xyz_f32_takes_the_pi_family_where_it_is_claimed():
    for c in H.CASES:
        if c["scene"] != "plain":
            continue
        e = H.euler_xyz_f32(H.case(c["name"])["truth"][:3, :3])
        if c["family"] == "pi":
            assert abs(e[0]) > 3.1 and abs(e[1]) > 3.1, (c["name"], e)
        else:
            assert abs(e[0]) < 0.02 and abs(e[1]) < 0.02, (c["name"], e)


@pytest.mark.parametrize("method", H.METHODS)
def test_every_case_is_one_the_reference_solves(method):
    """No case left out: from every case's guess the reference reports convergence and ends within the method's own bound of the truth."""
    bt, br = H.TRUTH_BOUND[method]
    failed = []
    for name in H.NAMES:
        c, r = H.case(name), H.reference(method, name)
        et, er = synth.pose_error(r["pose"], c["truth"])
        print(f"{method} {name}: converged {r['converged']} after {r['iterations']}, {et:.4f} m {er:.5f} rad from the truth")
        if not (r["converged"] and r["iterations"] >= 1 and np.isfinite(r["pose"]).all() and et < bt and er < br):
            failed.append((name, r["converged"], r["iterations"], et, er))
    assert not failed, failed


@pytest.mark.parametrize("method", ["gicp", "liorf"])
def test_recorded_references_are_a_fresh_runs(method):
    """tests/golden/heading_refs.npz (what the GPU tests read for the two numpy references) against the run above: the same verdicts and
    iteration counts; the poses are floats on both sides, equal but for the C library's last bit in a sine"""
    for name in H.NAMES:
        a, b = H.recorded_reference(method, name), H.reference(method, name)
        assert (a["converged"], a["iterations"]) == (b["converged"], b["iterations"]), name
        dt, dr = synth.pose_error(a["pose"], b["pose"])
        assert dt <= 2e-6 and dr <= 2e-6, (name, dt, dr)      # (a float ulp of the pose at 10 m is 1e-6: tests/test_gicp_gpu.py's bar for two loops)
