"""Every registration method at headings around the full circle (tests/heading_cases.py; tests/test_heading_cases.py shows on the CPU that
each case reaches the branch it claims and is one the references solve): one linearisation at the guess and one scan2Map from it, against
each method's exact reference with the helpers and tolerances of the method's own test file -- copied, no new number but one: the bound of
liorf's 6-DoF round trip, derived below.  The largest deviations are printed (pytest -s) and recorded in DESIGN.md, section 2."""
import numpy as np
import pytest

import gicp_ref
import heading_cases as H
import liorf_ref as R
import oracle
from simpleslam_amd import GicpRegister, LiorfRegister, LoamRegister, NdtRegister, VgicpRegister, pcr, synth

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4        # tests/test_loam_gpu.py:15-16, and the bar every other method's file holds its scan2Map to
POSE_TOL_RAD = 1e-4
SCENES = ["plain", "rot_x", "rot_y"]
SEEN = {}                # method -> {figure: largest value seen}, printed by the last test


def _note(method, **figures):
    for k, v in figures.items():
        SEEN.setdefault(method, {})[k] = max(float(v), SEEN.get(method, {}).get(k, 0.0))


def _make(method):
    if method == "loam":
        return LoamRegister(record_trace=1)
    if method == "ndt":
        return NdtRegister(ndt_resolution=H.NDT_RESOLUTION)
    return {"vgicp": VgicpRegister, "gicp": GicpRegister, "liorf": LiorfRegister}[method]()


def _kept(scene):
    """one handle per method with the scene's map as its kept target (the linearisations), and the map's covariances for the two GICPs"""
    regs = {m: _make(m) for m in H.METHODS}
    for reg in regs.values():
        reg.setTarget(H.scene_map(scene))
    return dict(regs=regs, tree=oracle.KdTree(H.scene_map(scene)), map_cov=H._map_covariances(scene))


@pytest.fixture(scope="module")
def plain(gpu):
    return _kept("plain")


@pytest.fixture(scope="module")
def rot_x(gpu):
    return _kept("rot_x")


@pytest.fixture(scope="module")
def rot_y(gpu):
    return _kept("rot_y")


@pytest.fixture(scope="module")
def aligners(gpu):
    """one handle per method for the scan2Map calls (the target is handed over with every call), and LOAM's co-resident variant"""
    regs = {m: _make(m) for m in H.METHODS}
    prm = pcr.default_params(record_trace=1)
    prm.loam_coresident = 1      # as tests/test_loam_head_gpu.py::test_coresident_variant switches
    regs["loam-coresident"] = LoamRegister(params=prm)
    return regs


def _scene(request, name):
    return request.getfixturevalue(H.BY_NAME[name]["scene"])


# ---- one linearisation at the guess ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.NAMES)
def test_loam_linearize(request, name):
    """tests/test_loam_gpu.py::_check_linearize"""
    s, c = _scene(request, name), H.case(name)
    for pose in (c["init"], c["truth"]):
        g = s["regs"]["loam"].linearize(c["scan"], pose, per_point=True)
        o = oracle.loam_linearize(s["tree"], c["scan"], pose, oracle.loam_params(), per_point=True)
        assert g["n"] == o["n"] and g["n"] > 1000
        np.testing.assert_array_equal(g["status"], o["status"])
        acc = o["status"] == 0
        np.testing.assert_array_equal(g["nn"][acc], o["nn"][acc])
        np.testing.assert_allclose(g["rows"][acc], o["rows"][acc], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(g["JtJ"], o["JtJ"], rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(g["JtE"], o["JtE"], rtol=1e-9, atol=1e-9)
        _note("loam", rows_not_bitwise=(g["rows"][acc] != o["rows"][acc]).sum(), JtJ_rel=np.abs(g["JtJ"] - o["JtJ"]).max() / np.abs(o["JtJ"]).max(),
              JtE_abs=np.abs(g["JtE"] - o["JtE"]).max())


@pytest.mark.parametrize("name", H.NAMES)
def test_vgicp_linearize(request, name):
    """tests/test_vgicp_gpu.py::test_linearize_matches_oracle"""
    s, c = _scene(request, name), H.case(name)
    sc = oracle.vgicp_covariances(c["scan"], 20, 8)
    g = s["regs"]["vgicp"].linearize(c["scan"], c["init"])
    o = oracle.vgicp_linearize(c["scan"], c["map"], c["init"], sc, s["map_cov"])
    assert g["n"] == o["n"] and g["n"] > 2000
    np.testing.assert_allclose(g["H"], o["H"], rtol=1e-7, atol=1e-6)
    np.testing.assert_allclose(g["b"], o["b"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g["err"], o["err"], rtol=1e-8)
    _note("vgicp", H_rel=np.abs(g["H"] - o["H"]).max() / np.abs(o["H"]).max(), b_abs=np.abs(g["b"] - o["b"]).max(), err_rel=abs(g["err"] - o["err"]) / abs(o["err"]))


@pytest.mark.parametrize("name", H.NAMES)
def test_gicp_linearize(request, name):
    """tests/test_gicp_gpu.py::check_linearisation"""
    s, c = _scene(request, name), H.case(name)
    scan = H.method_scan("gicp", c)
    CA, CB = H.gicp_covariances(name)
    ref = gicp_ref.linearize(scan, c["map"], c["init"], CA, CB, with_ambiguous=True)
    got = s["regs"]["gicp"].linearize(scan, c["init"], per_point=True)
    amb = ref["ambiguous"]
    assert amb.sum() < 0.01 * max(amb.size, 1), (name, int(amb.sum()))
    ok = ~amb
    np.testing.assert_array_equal(got["corr"][ok], ref["corr"][ok], err_msg=name)
    np.testing.assert_array_equal(got["d2"][ok].view(np.uint32), ref["d2"][ok].view(np.uint32), err_msg=name)
    if not amb.any():
        assert got["n"] == ref["n"], name
    same = ok & (got["corr"] == ref["corr"])
    dM = gicp_ref.m_diff(got["M"][same], ref["M"][same])
    dH, db, de = gicp_ref.sums_diff(got, ref)
    print(name, "n %d  M %.3g  H %.3g  b %.3g  err %.3g" % (ref["n"], dM, dH, db, de))
    _note("gicp", M=dM, H=dH, b=db, err=de)
    assert dM <= gicp_ref.DEVICE_M_BOUND, (name, dM)
    assert dH <= gicp_ref.DEVICE_H_BOUND and db <= gicp_ref.DEVICE_B_BOUND and de <= gicp_ref.DEVICE_ERR_BOUND, (name, dH, db, de)


def _ndt_close(a, b, what):
    """tests/test_ndt_sums_gpu.py::_close: a against b at the bars of tests/test_ndt_gpu.py::test_derivatives_match_oracle"""
    if "score" in a and "score" in b:
        assert abs(a["score"] - b["score"]) <= 1e-9 * abs(b["score"]), (what, a["score"], b["score"])
        assert np.abs(a["grad"] - b["grad"]).max() <= 1e-7 * np.abs(b["grad"]).max(), what
        _note("ndt", score_rel=abs(a["score"] - b["score"]) / abs(b["score"]), grad_rel=np.abs(a["grad"] - b["grad"]).max() / np.abs(b["grad"]).max())
    if "hess" in a and "hess" in b:
        assert np.abs(a["hess"] - b["hess"]).max() <= 1e-8 * np.abs(b["hess"]).max(), what
        _note("ndt", hess_rel=np.abs(a["hess"] - b["hess"]).max() / np.abs(b["hess"]).max())
    if "hess_d" in a and "hess_d" in b:
        assert np.abs(a["hess_d"] - b["hess_d"]).max() <= 1e-8 * np.abs(b["hess_d"]).max(), what
        _note("ndt", hess_d_rel=np.abs(a["hess_d"] - b["hess_d"]).max() / np.abs(b["hess_d"]).max())


@pytest.mark.parametrize("name", H.NAMES)
def test_ndt_derivatives(request, name):
    """p6 = (t, euler_xyz_f32(R)): both families of start parameters -- angles near 0 and angles near +-pi -- and the boundary, through the
    kernels of the host-driven loop and the three passes of the device-resident one.  At the truth (the family the case is named for) and at
    the guess (whose own roll may have either sign)."""
    s, c = _scene(request, name), H.case(name)
    reg = s["regs"]["ndt"]
    prm = oracle.ndt_params(resolution=H.NDT_RESOLUTION)
    for at in ("truth", "init"):
        p6 = H.ndt_p6(c[at])
        o = oracle.ndt_derivatives(c["scan"], c["map"], p6, prm, double_hessian=True)
        assert abs(o["score"]) > 100.0 and np.abs(o["grad"]).max() > 0 and np.abs(o["hess"]).max() > 0, (name, at)
        host = reg.derivatives(c["scan"], p6, double_hessian=True)
        _ndt_close(host, o, (name, at, "host", "oracle"))
        for kind in (0, 1, 2):
            got = reg.derivatives(c["scan"], p6, device_loop=True, kind=kind)
            _ndt_close(got, o, (name, at, "device", kind, "oracle"))
            _ndt_close(got, host, (name, at, "device", kind, "host"))


@pytest.mark.parametrize("name", H.NAMES)
def test_liorf_linearize(request, name):
    """tests/test_liorf_gpu.py::test_linearize_matches_the_reference, at pcr.liorf_pose_to_6dof of the guess"""
    s, c = _scene(request, name), H.case(name)
    scan = H.method_scan("liorf", c)
    six = pcr.liorf_pose_to_6dof(c["init"])
    o = s["regs"]["liorf"].linearize(scan, six)
    assert np.abs(o["T"] - R.transformation(six)).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(o["T"]).max())
    pp = R.per_point(scan, c["map"], o["T"], R.row_trig(six))
    assert np.array_equal(o["kept"], pp["kept"]) and pp["kept"].sum() > 500
    assert o["n"] == int(pp["kept"].sum())
    k = pp["kept"]
    assert np.allclose(o["coeff"][k], pp["coeff"][k], rtol=1e-5, atol=0)
    assert np.array_equal(o["coeff"], pp["coeff"])
    assert not o["coeff"][~k].any()
    AtA, AtB = R.sums(pp["rows"], pp["coeff"], pp["kept"])
    dA, dB = np.abs(o["AtA"] - AtA).max() / np.abs(AtA).max(), np.abs(o["AtB"] - AtB).max() / np.abs(AtB).max()
    print(name, "AtA rel", dA, "AtB rel", dB)
    _note("liorf", AtA_rel=dA, AtB_rel=dB)
    assert dA <= 1e-6 and dB <= 1e-6


# liorf's two PCL formulas, pose -> six numbers -> pose.  The float32 restatement (tests/liorf_ref.py) differs from the float64 one below by at most
# 1.278e-07 in an entry over the truths and guesses of these cases (measured by this test, which prints it; the translation is copied, so the
# largest entries that are computed are the rotation's, up to 1: about two float32 ulps of them).  Four times that, since the order of operations
# inside cosf and sinf differs between C libraries: a few float32 ulps of the largest entry.
SIXDOF_SPREAD = 1.278e-07
SIXDOF_BOUND = 4 * SIXDOF_SPREAD


def _sixdof_f64(T):
    t = np.asarray(T, np.float64).astype(np.float32).astype(np.float64)
    roll, pitch, yaw = np.arctan2(t[2, 1], t[2, 2]), np.arcsin(-t[2, 0]), np.arctan2(t[1, 0], t[0, 0])
    A, B, Cc, D, E, Fs = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    out = np.eye(4)
    out[0] = [A * Cc, A * D * Fs - B * E, B * Fs + A * D * E, t[0, 3]]
    out[1] = [B * Cc, A * E + B * D * Fs, B * D * E - A * Fs, t[1, 3]]
    out[2] = [-D, Cc * Fs, Cc * E, t[2, 3]]
    return out, np.array([roll, pitch, yaw])


def test_liorf_six_dof_round_trip(gpu):
    """atan2f wraps at yaw +-180 degrees and roll is about pi with the sensor upside down: the pose that comes back is the one that went in"""
    spread = worst = 0.0
    for name in H.NAMES:
        c = H.case(name)
        for T in (c["truth"], c["init"]):
            want, angles = _sixdof_f64(T)
            spread = max(spread, float(np.abs(R.transformation(R.pose_to_6dof(T)).astype(np.float64) - want).max()))
            six = pcr.liorf_pose_to_6dof(T)
            d_ang = np.abs((six[:3].astype(np.float64) - angles + np.pi) % (2 * np.pi) - np.pi)      # (an angle next to pi may come back as -pi)
            assert d_ang.max() <= 4 * np.finfo(np.float32).eps * np.pi, (name, six, angles)
            got = pcr.liorf_6dof_to_pose(six)
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.abs(got - want).max() <= SIXDOF_BOUND, (name, np.abs(got - want).max())
    print(f"liorf 6-DoF round trip: float32 restatement {spread:.3e}, library {worst:.3e} from the float64 restatement")
    _note("liorf", sixdof=worst)
    assert spread <= 2 * SIXDOF_SPREAD      # the recorded figure is still what the restatement measures (another C library may move a last bit)
    yaws = [abs(pcr.liorf_pose_to_6dof(H.case(n)["truth"])[2]) for n in H.NAMES]
    rolls = [abs(pcr.liorf_pose_to_6dof(H.case(n)["truth"])[0]) for n in H.NAMES]
    assert sum(y > 3.13 for y in yaws) >= 6 and sum(r > 3.1 for r in rolls) >= 2      # the wrap and the upside-down sensor are among the cases


# ---- one scan2Map from the guess -------------------------------------------------------------------------------------------------------------
def _check_pose(method, name, pose, ref):
    dt, dr = synth.pose_error(pose, ref["pose"])
    print(f"{method} {name}: {ref['iterations']} iterations, {dt:.3e} m {dr:.3e} rad from the reference")
    _note(method, pose_m=dt, pose_rad=dr)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (method, name, dt, dr)


def _loam_scan2map(reg, name):
    c, ref = H.case(name), H.reference("loam", name)
    pose = c["init"].copy()
    conv = reg.scan2Map(c["scan"], c["map"], pose)
    tr = reg.trace()
    assert conv == ref["converged"] and tr["iters_run"] == ref["iterations"]
    np.testing.assert_array_equal(tr["n"], ref["n"])
    _check_pose("loam", name, pose, ref)
    R3 = pose[:3, :3]
    assert np.abs(R3.T @ R3 - np.eye(3)).max() < 1e-14 and H.t2se3_route(R3) == c["route"]      # the pose left through t2se3, by the claimed route
    return pose


@pytest.mark.parametrize("name", H.NAMES)
def test_loam_scan2map(aligners, name):
    _loam_scan2map(aligners["loam"], name)


@pytest.mark.parametrize("name", H.VARIANT_CASES)
def test_loam_scan2map_coresident_variant(aligners, name):
    """t2se3 sits in the shared tail of both instantiations of the iterate kernel: i = 0, 1 and 2 under the co-resident one, bit for bit the default's"""
    pose = _loam_scan2map(aligners["loam-coresident"], name)
    base = H.case(name)["init"].copy()
    aligners["loam"].scan2Map(H.case(name)["scan"], H.case(name)["map"], base)
    np.testing.assert_array_equal(pose, base)


@pytest.mark.parametrize("name", H.NAMES)
@pytest.mark.parametrize("method", ["vgicp", "gicp", "ndt", "liorf"])
def test_scan2map(aligners, method, name):
    c, ref = H.case(name), H.recorded_reference(method, name)
    reg = aligners[method]
    pose = c["init"].copy()
    conv = reg.scan2Map(H.method_scan(method, c), c["map"], pose)
    assert np.isfinite(pose).all()
    assert conv == ref["converged"], (method, name)
    assert reg.stats()["iterations"] == ref["iterations"], (method, name)
    _check_pose(method, name, pose, ref)
    if method == "ndt":
        _note("ndt", pose_not_bitwise=not np.array_equal(pose, ref["pose"]))


def test_print_the_largest_deviations():
    for method in sorted(SEEN):
        print(method, " ".join(f"{k} {v:.3g}" for k, v in sorted(SEEN[method].items())))
