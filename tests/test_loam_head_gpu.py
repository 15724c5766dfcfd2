"""The head of a LOAM Gauss-Newton launch -- fold of the partial sums, 6x6 solve by lane permutes, the wave-wide pose update -- at the smallest shapes
that reach each of its branches, against the CPU oracle (oracle.loam_scan2map) at the tolerance of tests/test_loam_gpu.py.

Shapes: 300 points = two blocks, the second partly filled (one fold pass, rows masked past the end); 70 000 points = 274 blocks, so the fold takes
its second loop (rows 256..273); a single plane = a pivot collapses and the LDLT fallback answers (that case on the suite's 8 192-point scan)."""
import functools

import numpy as np
import pytest

import oracle
from simpleslam_amd import LoamRegister, pcr, synth

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4
POSE_TOL_RAD = 1e-4


@functools.lru_cache(maxsize=None)
def _scene(n_scan):
    scan, m, T = synth.plane_scene("corner", n_map=20000, n_scan=n_scan, seed=3)
    w = dict(scan=scan, map=m, truth=T, init=synth.perturb(T, 3, trans=0.1, rot_deg=1.0))
    for v in w.values():
        v.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _oracle(n_scan, iters, early_exit):
    w = _scene(n_scan)
    return oracle.loam_scan2map(w["scan"], w["map"], w["init"], oracle.loam_params(iters=iters, early_exit=early_exit), trace=True)


def _run(w, **kw):
    reg = LoamRegister(**kw)
    pose = w["init"].copy()
    conv = reg.scan2Map(w["scan"], w["map"], pose)
    return reg, pose, conv


def _check_pose(pose, po):
    dt, dr = synth.pose_error(pose, po)
    print(f"pose against the oracle: {dt:.3e} m, {dr:.3e} rad")
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dt, dr)


def test_two_blocks_second_partly_filled(gpu):
    w = _scene(300)
    po, co, info = _oracle(300, 10, 0)
    reg, pose, conv = _run(w, loam_iters=10, loam_early_exit=0, record_trace=1)
    assert conv == co
    tr = reg.trace()
    assert tr["iters_run"] == info["iters_run"] == 10
    np.testing.assert_array_equal(tr["n"], info["n"])
    _check_pose(pose, po)
    # bitwise repeatable over three calls
    for _ in range(2):
        again = w["init"].copy()
        reg.scan2Map(w["scan"], w["map"], again)
        np.testing.assert_array_equal(again, pose)
    # the sums of one linearisation equal those of the same call repeated
    lin = LoamRegister()
    lin.setTarget(w["map"])
    a = lin.linearize(w["scan"], w["init"])
    b = lin.linearize(w["scan"], w["init"])
    assert a["n"] == b["n"] > 6
    np.testing.assert_array_equal(a["JtJ"], b["JtJ"])
    np.testing.assert_array_equal(a["JtE"], b["JtE"])


def test_more_than_256_partial_rows(gpu):
    w = _scene(70000)
    po, co, info = _oracle(70000, 4, 0)
    reg, pose, conv = _run(w, loam_iters=4, loam_early_exit=0, record_trace=1)
    tr = reg.trace()
    assert conv == co and tr["iters_run"] == info["iters_run"] == 4
    np.testing.assert_array_equal(tr["n"], info["n"])
    _check_pose(pose, po)
    again = w["init"].copy()
    reg.scan2Map(w["scan"], w["map"], again)
    np.testing.assert_array_equal(again, pose)


def test_weak_pivot_takes_the_ldlt_fallback(gpu, world_small):
    """A single plane leaves three degrees of freedom free: a pivot collapses and the step is the oracle's pivoted LDLT's (the geometry and the
    tolerance of tests/test_loam_gpu.py; the pose after the step is exp of a huge rotation and not comparable).  A scan that lies flat in a
    flat map does not serve here: its free components are rounding noise of the sums' order on both sides (GPU and oracle differ by 4 % there,
    before and after this file's changes)."""
    rng = np.random.default_rng(3)
    plane = np.zeros((20000, 4), np.float32)
    plane[:, 0] = rng.uniform(-20, 20, 20000); plane[:, 1] = rng.uniform(-20, 20, 20000); plane[:, 2] = -1.5
    scan = world_small["scan"]
    reg = LoamRegister(loam_iters=1, loam_early_exit=0, record_trace=1)
    pose = np.eye(4)
    conv = reg.scan2Map(scan, plane, pose)
    po, co, info = oracle.loam_scan2map(scan, plane, np.eye(4), oracle.loam_params(iters=1, early_exit=0), trace=True)
    tr = reg.trace()
    assert conv == co and tr["iters_run"] == info["iters_run"] == 1
    np.testing.assert_array_equal(tr["n"], info["n"][:1])
    assert np.isfinite(tr["x"][0]).all()
    np.testing.assert_allclose(tr["x"][0], info["x"][0], rtol=1e-6, atol=1e-9)


def test_early_exit_on_and_off(gpu):
    w = _scene(300)
    po, co, info = _oracle(300, 10, 1)
    assert co and 2 <= info["iters_run"] < 10          # the case is one that converges early: the later launches leave through prev_done
    reg, pose, conv = _run(w, loam_iters=10, loam_early_exit=1, record_trace=1)
    assert conv == co
    assert reg.trace()["iters_run"] == info["iters_run"]
    _check_pose(pose, po)
    po0, co0, info0 = _oracle(300, 10, 0)
    reg, pose, conv = _run(w, loam_iters=10, loam_early_exit=0, record_trace=1)
    assert conv == co0 == False and reg.trace()["iters_run"] == info0["iters_run"] == 10
    _check_pose(pose, po0)


def test_trace_is_filled_on_every_iteration(gpu):
    w = _scene(300)
    po, co, info = _oracle(300, 10, 0)
    reg, pose, conv = _run(w, loam_iters=10, loam_early_exit=0, record_trace=1)
    tr = reg.trace()
    assert tr["iters_run"] == 10
    np.testing.assert_array_equal(tr["n"], info["n"])
    np.testing.assert_allclose(tr["JtJ"], info["JtJ"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(tr["JtE"], info["JtE"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(tr["x"], info["x"], rtol=1e-6, atol=1e-12)
    # and recording the trace changes nothing: the matrix is unpacked only for it
    _, quiet, _ = _run(w, loam_iters=10, loam_early_exit=0)
    np.testing.assert_array_equal(quiet, pose)


def test_coresident_variant(gpu):
    w = _scene(300)
    po, co, info = _oracle(300, 10, 0)
    prm = pcr.default_params(loam_iters=10, loam_early_exit=0)
    prm.loam_coresident = 1
    reg = LoamRegister(params=prm)
    pose = w["init"].copy()
    conv = reg.scan2Map(w["scan"], w["map"], pose)
    assert conv == co
    _check_pose(pose, po)
    _, base, _ = _run(w, loam_iters=10, loam_early_exit=0)
    np.testing.assert_array_equal(pose, base)
