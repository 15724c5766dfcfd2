"""pcr_deskew_host (the definition of the deskew: csrc/deskew_math.h on host memory, no GPU) against the numpy restatement tests/deskew_ref.py, bit
for bit on the shared cases; its refusals; what it means (points of a moving sensor come back to where a resting one would have seen them); and the
bound the header states for normalised linear interpolation against constant angular velocity."""
import os
import subprocess

import numpy as np
import pytest

import deskew_cases
import deskew_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "simpleslam_amd", "lib", "deskew_check")
CASES = deskew_cases.all_cases()


@pytest.fixture(scope="module")
def reference():
    """The numpy restatement of every case, computed once."""
    return {c["name"]: deskew_ref.deskew(c["cloud"], c["poses"], c["stamps"], c["times"], c["kind"], c["offset"], c["t0"], c["t_ref"]) for c in CASES}


def run_host(c):
    from simpleslam_amd import deskew_host
    cloud = c["cloud"].copy()
    out = cloud if c["inplace"] else None
    return deskew_host(cloud, c["poses"], c["stamps"], c["times"], c["kind"], c["offset"], c["t0"], c["t_ref"], out=out)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_the_numpy_restatement(case, reference):
    out, info = run_host(case)
    want, want_info = reference[case["name"]]
    np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32))
    assert info == want_info
    assert info["ref_clamped"] == case["expect_ref_clamped"]
    if case["cloud"].shape[0] >= 63:      # (the special records of deskew_cases.make_case)
        assert info["before"] >= 1 and info["after"] >= 1 and info["nonfinite"] >= 2
        moved = (out.view(np.uint32)[:, :3] != case["cloud"].view(np.uint32)[:, :3]).any(1)
        assert moved[8:].all() and not moved[6] and not moved[7]
        np.testing.assert_array_equal(out.view(np.uint32)[:, 3:], case["cloud"].view(np.uint32)[:, 3:])


def test_the_cases_cover_the_quaternion_rules():
    by = {c["name"]: c for c in CASES}
    assert deskew_cases.negative_dot_somewhere(by["n4099_K17_flip_stride20"])
    assert deskew_cases.non_positive_trace_somewhere(by["n257_K3_trace"])
    assert {c["kind"] for c in CASES} == {0, 1, 2}
    assert {c["cloud"].shape[0] for c in CASES} == {1, 63, 64, 65, 255, 256, 257, 4099}
    assert {c["poses"].shape[0] for c in CASES} == {2, 3, 17, 1024}


def test_identity_motion_returns_the_input():
    from simpleslam_amd import deskew_host
    c = CASES[7]
    poses = np.tile(np.eye(4), (5, 1, 1))
    out, info = deskew_host(c["cloud"], poses, [0.0, 0.01, 0.05, 0.2, 0.3], times=np.linspace(-0.1, 0.4, c["cloud"].shape[0]), t_ref=0.123)
    np.testing.assert_array_equal(out.view(np.uint32), c["cloud"].view(np.uint32))
    assert info["before"] > 0 and info["after"] > 0 and info["nonfinite"] == 2


@pytest.mark.parametrize("name,word,change", deskew_cases.refusals(), ids=[r[0] for r in deskew_cases.refusals()])
def test_refusals_name_the_field_and_write_nothing(name, word, change):
    kw = dict(deskew_cases.good_call(), **change)
    out = np.full_like(kw["cloud"], -77.0)
    rc, msg = deskew_cases.raw_call(out=out, **kw)
    assert rc != 0 and word in msg, msg
    assert (out == -77.0).all()


def test_overlap_and_empty_input():
    kw = deskew_cases.good_call()
    buf = np.zeros((10, 8), np.float32)
    buf[:7] = kw["cloud"]
    keep = buf.copy()
    rc, msg = deskew_cases.raw_call(out=buf[2:], **dict(kw, cloud=buf[:7]))
    assert rc != 0 and "out overlaps pts" in msg and (buf == keep).all()
    tbuf = np.zeros(64, np.float32)
    rc, msg = deskew_cases.raw_call(out=tbuf.view(np.float32), **dict(kw, times=tbuf[:7]))
    assert rc != 0 and "out overlaps times" in msg
    rc, msg = deskew_cases.raw_call(out=buf, **dict(kw, cloud=buf[:7]))      # in place is no overlap
    assert rc == 0, msg
    rc, msg = deskew_cases.raw_call(out=buf, **dict(kw, cloud=buf[:0], times=tbuf[:0], null=("pts", "out")))      # n == 0 succeeds, whatever the pointers
    assert rc == 0, msg


def constant_twist_pose(start, v, w, t):
    from simpleslam_amd import synth
    return start @ synth.se3_exp(np.concatenate([v, w]) * t)


def test_deskewed_points_are_where_a_resting_sensor_sees_them():
    """World points below 64 m, a trajectory of 11 poses over 0.1 s at 2 m/s and 0.5 rad/s.  Each point is expressed in the sensor frame at its own
    time (numpy f64, the same interpolation), rounded to float and deskewed: every coordinate must come back within 1e-5 m of the point in the frame
    at t_ref.  The limit: float spacing below 64 m is 3.8e-6 m, so the input rounding is at most 1.9e-6 m per coordinate, at most 3.3e-6 m after a
    rotation; the output rounding adds at most 1.9e-6 m: 5.2e-6 m in all."""
    from simpleslam_amd import deskew_host
    rng = np.random.default_rng(20261021)
    n = 5000
    stamps = np.linspace(0.0, 0.1, 11)
    start = constant_twist_pose(np.eye(4), [3.0, -2.0, 0.5], [0.02, -0.01, 0.7], 1.0)
    poses = np.stack([constant_twist_pose(start, [2.0, 0.0, 0.0], [0.0, 0.0, 0.5], t) for t in stamps])
    t_ref = 0.1
    tab = deskew_ref.table(poses, stamps)
    times = rng.uniform(0.0, 0.1, n)
    R, p, _ = deskew_ref.evaluate(tab, times)
    Rr, pr, _ = deskew_ref.evaluate(tab, [t_ref])
    # world points such that every coordinate stays below 64 m in both frames: drawn in the reference frame within 36 m (36 sqrt(3) < 63)
    in_ref = rng.uniform(-36.0, 36.0, (n, 3))
    world = in_ref @ Rr[0].T + pr[0]
    in_own = np.einsum("nji,nj->ni", R, world - p)      # R^T (w - p)
    assert np.abs(in_own).max() < 64.0 and np.abs(in_ref).max() < 64.0
    cloud = np.zeros((n, 4), np.float32)
    cloud[:, :3] = in_own
    out, info = deskew_host(cloud, poses, stamps, times=times, time_kind=2, t_ref=t_ref)
    err = np.abs(out[:, :3].astype(np.float64) - in_ref).max()
    moved = np.abs(cloud[:, :3].astype(np.float64) - in_ref).max()
    print(f"largest coordinate error {err:.3e} m (undeskewed: {moved:.3e} m)")
    assert err <= 1e-5
    assert moved > 0.05      # (the motion is worth taking out)
    assert info == dict(before=0, after=0, nonfinite=0, ref_clamped=0)


def _angle(Ra, Rb):
    Rr = np.einsum("nji,njk->nik", Ra, Rb)
    c = (np.trace(Rr, axis1=1, axis2=2) - 1) / 2
    s = 0.5 * np.sqrt((Rr[:, 2, 1] - Rr[:, 1, 2]) ** 2 + (Rr[:, 0, 2] - Rr[:, 2, 0]) ** 2 + (Rr[:, 1, 0] - Rr[:, 0, 1]) ** 2)
    return np.arctan2(s, c)


@pytest.mark.parametrize("theta", [0.01, 0.03, 0.1, np.deg2rad(3.0), np.deg2rad(10.0), 0.3, 0.5, 0.75, 1.0])
def test_nlerp_stays_within_theta_cubed_over_240_of_constant_rate(theta):
    """The header's interpolation (through pcr_deskew_host: a point on each axis at every s of a fine grid gives the interpolated rotation's columns)
    against the rotation of constant angular velocity, over one segment that turns by theta about a skew axis."""
    from simpleslam_amd import deskew_host, synth
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    start = synth.se3_exp([0, 0, 0, 0.4, 0.2, -0.3])
    poses = np.stack([start, start @ synth.se3_exp(np.concatenate([[0, 0, 0], axis * theta]))])
    s = np.linspace(0.0, 1.0, 2001)
    cloud = np.zeros((3 * len(s), 4), np.float32)
    cloud[0::3, 0] = cloud[1::3, 1] = cloud[2::3, 2] = 1.0
    # t_ref = 0: the output is start^T R(s) e_k -- column k of the rotation relative to the segment's start
    out, _ = deskew_host(cloud, poses, [0.0, 1.0], times=np.repeat(s, 3), time_kind=2, t_ref=0.0)
    got = out[:, :3].astype(np.float64).reshape(len(s), 3, 3).transpose(0, 2, 1)
    want = np.stack([synth.se3_exp(np.concatenate([[0, 0, 0], axis * theta * si]))[:3, :3] for si in s])
    bound = theta ** 3 / 240
    # in double, through the restatement that the cases above pin to the library bit for bit: the bound itself
    R, _, _ = deskew_ref.evaluate(deskew_ref.table(poses, [0.0, 1.0]), s)
    exact = _angle(np.einsum("ji,njk->nik", start[:3, :3], R), want).max()
    # through the library: the columns come back as floats, 6e-8 per entry, at most 1.5e-7 rad of angle on top of the bound
    worst = _angle(got, want).max()
    print(f"theta {theta:.4f}: worst {exact:.3e} rad (through float output {worst:.3e}), bound {bound:.3e} rad = theta^3 / 240; worst = theta^3 / {theta ** 3 / exact:.1f}")
    assert exact <= bound
    assert worst <= bound + 1.5e-7


def test_the_check_program():
    assert os.path.exists(CHECK), "deskew_check not built (run __graft_entry__.build())"
    out = subprocess.run([CHECK, "--self"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAILED" not in out.stdout
