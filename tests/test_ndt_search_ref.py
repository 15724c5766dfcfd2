"""The yardstick of tests/test_ndt_search_gpu.py, checked on the CPU: tests/ndt_search_ref.py (the numpy restatement of pclomp's per-pair
terms with the three neighbourhood tables) against oracle/ndt_oracle.c where the two overlap -- DIRECT7 -- and the inputs of the GPU
end-to-end test.  Nothing here runs the device; these tests pass with or without the ndt_search setting."""
import numpy as np
import pytest

import ndt_clouds as nc
import ndt_search_ref as sr
import oracle

P6 = np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.015])


@pytest.fixture(scope="module")
def room_target():
    return sr.Target(nc.room())


def _close(a, o, what):
    """the bars of test_ndt_gpu.py::test_derivatives_match_oracle"""
    assert abs(a["score"] - o["score"]) <= 1e-9 * abs(o["score"]), what
    assert np.abs(a["grad"] - o["grad"]).max() <= 1e-7 * np.abs(o["grad"]).max(), what
    assert np.abs(a["hess"] - o["hess"]).max() <= 1e-8 * np.abs(o["hess"]).max(), what


@pytest.mark.parametrize("n", nc.ROOM_SCAN_SIZES)
def test_reference_equals_the_oracle_under_direct7_on_the_room(room_target, n):
    m, scan, _ = nc.room_scan_case(n)
    o = oracle.ndt_derivatives(scan, m, P6, double_hessian=True)
    assert abs(o["score"]) > 1.0
    full = sr.sums(room_target, scan, P6, sr.DIRECT7, 0)
    _close(full, o, n)
    light = sr.sums(room_target, scan, P6, sr.DIRECT7, 1)
    assert light["score"] == full["score"] and np.array_equal(light["grad"], full["grad"]) and "hess" not in light
    hd = sr.sums(room_target, scan, P6, sr.DIRECT7, 2)["hess_d"]
    assert np.abs(hd - o["hess_d"]).max() <= 1e-8 * np.abs(o["hess"]).max()


@pytest.mark.parametrize("leaf", nc.FACES_LEAVES)
def test_reference_equals_the_oracle_under_direct7_at_voxel_faces(leaf):
    cloud, probes = nc.faces(leaf)
    prm = oracle.ndt_params(resolution=leaf)
    tg = sr.Target(cloud, prm)
    p0 = np.zeros(6)
    for i in range(len(probes)):
        q = probes[i:i + 1]
        o = oracle.ndt_derivatives(q, cloud, p0, prm, double_hessian=True)
        assert abs(o["score"]) > 0
        _close(sr.sums(tg, q, p0, sr.DIRECT7, 0), o, (leaf, i))
        hd = sr.sums(tg, q, p0, sr.DIRECT7, 2)["hess_d"]
        assert np.abs(hd - o["hess_d"]).max() <= 1e-8 * np.abs(o["hess"]).max(), (leaf, i)


def test_offset_tables():
    t26 = sr.offsets(sr.DIRECT26)
    assert t26.shape == (26, 3)
    cells = {tuple(int(v) for v in d) for d in t26}
    assert len(cells) == 26 and (0, 0, 0) not in cells                     # distinct, non-zero
    assert all((-a, -b, -c) in cells for a, b, c in cells)                 # closed under negation
    assert np.abs(t26).max() == 1                                          # inside the 3 x 3 x 3 block
    assert cells == {(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)} - {(0, 0, 0)}
    assert [tuple(d) for d in t26[:3]] == [(-1, -1, -1), (-1, 0, -1), (-1, 1, -1)] and tuple(t26[12]) == (-1, 0, 0)
    assert np.array_equal(t26[13:], -t26[:13])
    t7 = {tuple(int(v) for v in d) for d in sr.offsets(sr.DIRECT7)}
    assert len(t7) == 7 and (0, 0, 0) in t7 and all(sum(abs(v) for v in d) <= 1 for d in t7)
    assert [tuple(d) for d in sr.offsets(sr.DIRECT1)] == [(0, 0, 0)]
    with pytest.raises(ValueError):
        sr.offsets(sr.KDTREE)


def test_driven_optimiser_reproduces_the_oracle_under_direct7(room_target):
    """validates the driver: pcr_ndt_opt_* fed with this reference's DIRECT7 sums arrives where the oracle's own loop does"""
    m, scan, init = nc.room_scan_case(513)
    po, co, info = oracle.ndt_scan2map(scan, m, init)
    pose, conv, its, _ = sr.scan2map(room_target, scan, init, sr.DIRECT7)
    assert conv == co and its == info["iterations"]
    np.testing.assert_allclose(pose, po, rtol=0, atol=2e-6)      # (a float ulp of the pose; normally bit for bit)


@pytest.mark.parametrize("search", [sr.DIRECT1, sr.DIRECT26], ids=["DIRECT1", "DIRECT26"])
def test_end_to_end_inputs_converge_and_are_stable(room_target, search):
    """The inputs of test_ndt_search_gpu.py's end-to-end test: the reference-driven optimiser converges in at least 3 iterations, and its
    iteration count does not change when every sum it is fed is scaled by 1 +- 1e-9 -- a difference within the bars of a pass cannot flip
    a decision of the line search on these inputs."""
    m, scan, guess = sr.e2e_case(search)
    pose, conv, its, passes = sr.scan2map(room_target, scan, guess, search)
    print(f"{sr.NAMES[search]}: seed/trans/rot {sr.E2E_GUESS[search]}: converged {conv}, {its} iterations, {passes} passes")
    assert conv and its >= 3 and np.isfinite(pose).all()
    for scale in (1.0 + 1e-9, 1.0 - 1e-9):
        p2, c2, i2, n2 = sr.scan2map(room_target, scan, guess, search, scale=scale)
        assert (c2, i2, n2) == (conv, its, passes), scale
        assert np.abs(p2 - pose).max() <= 1e-5, scale
