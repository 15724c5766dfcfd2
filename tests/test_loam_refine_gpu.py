"""The refinement behind the LOAM neighbour search (loam_point between the search and the row): exact distances of the listed
eight, their (distance, index) order with the sorting network skipped when the order already holds, the proof, the plane fit
and the cache entry a launch leaves for the next one.  Everything is compared with the CPU oracle through the helper and the
tolerances of test_loam_gpu.py.

Shapes: 300-point scans (one full block of 256 and one with 44 valid lanes) against maps of 3 000 - 6 000 points, and 8-point
scans where the wave-per-query route has to be reached in a single linearisation (it serves blocks with <= 8 misses)."""
import numpy as np
import pytest

import oracle
from simpleslam_amd import LoamRegister, synth
from test_loam_gpu import POSE_TOL_M, POSE_TOL_RAD, _check_linearize

pytestmark = pytest.mark.gpu


def _cloud(xyz):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def _lattice(nx, ny, step=0.25, z=0.0, x0=0.0, y0=0.0):
    """points on an exact planar lattice: every coordinate is a multiple of `step` (a power of two), so symmetric distances tie in f64"""
    gx, gy = np.meshgrid(np.arange(nx) * step + x0, np.arange(ny) * step + y0, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], axis=1)


@pytest.fixture(scope="module")
def room():
    """Floor and two walls on jittered 0.25 m grids (3 675 points) and a 300-point scan of them: three orthogonal planes
    constrain all six degrees of freedom, and every scan point has five neighbours inside the gate."""
    rng = np.random.default_rng(11)
    floor = _lattice(49, 49, 0.25, 0.0, -6.0, -6.0)
    wall_x = _lattice(49, 13, 0.25)[:, [2, 0, 1]] + np.array([6.0, -6.0, 0.0])
    wall_y = _lattice(49, 13, 0.25)[:, [0, 2, 1]] + np.array([-6.0, 6.0, 0.0])
    m = np.concatenate([floor, wall_x, wall_y])
    m = m + rng.uniform(-0.05, 0.05, m.shape)
    f = np.stack([rng.uniform(-5, 5, 150), rng.uniform(-5, 5, 150), np.zeros(150)], axis=1)
    wx = np.stack([np.full(75, 6.0), rng.uniform(-5, 5, 75), rng.uniform(0.5, 2.5, 75)], axis=1)
    wy = np.stack([rng.uniform(-5, 5, 75), np.full(75, 6.0), rng.uniform(0.5, 2.5, 75)], axis=1)
    world_pts = np.concatenate([f, wx, wy])[rng.permutation(300)] + rng.normal(0, 0.005, (300, 3))
    T = np.eye(4)
    T[:3, 3] = [0.3, -0.2, 1.5]
    scan = _cloud((world_pts - T[:3, 3]) @ T[:3, :3])
    return dict(map=_cloud(m), scan=scan, truth=T)


def test_ties_decided_by_the_original_index(gpu):
    """Queries at symmetric positions over an exact 0.25 m lattice: at a cell centre neighbours 5-12 are equidistant in f64, over
    an edge midpoint 3-6 and 7-8, over a lattice point 2-5 and 6-9 -- the (distance, index) order decides, the ninth ties with the
    eighth (the proof fails, the exact scan decides).  Those queries fill the first wave, whose lanes need the sorting network; the
    other waves hold queries at generic positions, arrive ordered and skip it."""
    rng = np.random.default_rng(5)
    m = _lattice(64, 64, 0.25, 0.0, 0.0, 0.0)
    m = m[rng.permutation(len(m))]                   # the index order is unrelated to the position
    base = np.stack([rng.integers(8, 56, 64), rng.integers(8, 56, 64)], axis=1) * 0.25
    off = np.array([[0.125, 0.125], [0.125, 0.0], [0.0, 0.0], [0.0, 0.125]])[np.arange(64) % 4]
    sym = np.concatenate([base + off, np.full((64, 1), 0.0625)], axis=1)
    gen = np.stack([rng.uniform(2, 14, 236), rng.uniform(2, 14, 236), rng.uniform(0.02, 0.2, 236)], axis=1)
    scan, target = _cloud(np.concatenate([sym, gen])), _cloud(m)
    reg = LoamRegister()
    reg.setTarget(target)
    tree = oracle.KdTree(target)
    g, o, _ = _check_linearize(reg, tree, scan, np.eye(4))
    idx, d2 = tree.knn(scan[:, :3].astype(np.float64), 9)
    assert (d2[:64, 4] == d2[:64, 5]).sum() >= 32 and (d2[:64, 7] == d2[:64, 8]).sum() >= 32     # the ties are really there
    found = d2[:, 4] < 1.0
    assert found.all()
    np.testing.assert_array_equal(g["status"] != 1, found)
    np.testing.assert_array_equal(g["nn"], idx[:, :5])       # the five indices, exactly, for EVERY query


def test_every_route_of_the_search(gpu, room):
    """scan2map from a large, two medium and a small perturbation (first steps, as |rho| + 10 m |omega| from the oracle's trace:
    0.50, about 0.08 and 0.02 m; above 0.12 m a launch searches every query, at 0.02 m almost none).  Per launch the trace must show each regime of the miss exchange:
    two blocks (256 + 44 lanes) share S searches, so S > 172 means a block with > 128 misses, 17 <= S <= 128 one with 9 - 128
    and 1 <= S <= 8 one with <= 8.  A run in which a regime does not occur fails."""
    seen = []
    for trans, rot in ((0.25, 2.0), (0.05, 0.2), (0.03, 0.3), (0.01, 0.05)):
        T0 = synth.perturb(room["truth"], 7, trans=trans, rot_deg=rot)
        reg = LoamRegister(loam_iters=6, loam_early_exit=0, record_trace=1)
        pose = T0.copy()
        conv = reg.scan2Map(room["scan"], room["map"], pose)
        po, co, info = oracle.loam_scan2map(room["scan"], room["map"], T0, oracle.loam_params(iters=6, early_exit=0), trace=True)
        tr = reg.trace()
        print("searches per launch:", tr["searches"], "accepted:", tr["n"])
        assert conv == co and tr["iters_run"] == info["iters_run"]
        np.testing.assert_array_equal(tr["n"], info["n"][: tr["iters_run"]])
        dt, dr = synth.pose_error(pose, po)
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dt, dr)
        seen += [int(s) for s in tr["searches"]]
    assert any(s > 172 for s in seen), seen
    assert any(17 <= s <= 128 for s in seen), seen
    assert any(1 <= s <= 8 for s in seen), seen


def test_crowded_block_falls_back_from_the_wave_route(gpu, room):
    """A 1 m cell neighbourhood with more candidates than the wave table holds (kWaveTab = 280).  An 8-point scan posts <= 8 misses,
    which is what sends a block down the wave-per-query route in a single linearisation: with the crowded map the route reports
    fallback and the per-lane search decides, with the plain map the wave route itself answers.  The 300-point scan checks the
    per-lane route on the same map."""
    rng = np.random.default_rng(2)
    blob = np.array([1.5, 1.5, 0.0]) + np.concatenate([rng.uniform(-0.4, 0.4, (500, 2)), rng.normal(0, 0.01, (500, 1))], axis=1)
    crowded = np.concatenate([room["map"], _cloud(blob)])
    T = room["truth"]
    near = np.stack([rng.uniform(1.2, 1.8, 8), rng.uniform(1.2, 1.8, 8), rng.normal(0, 0.01, 8)], axis=1)
    few = _cloud((near - T[:3, 3]) @ T[:3, :3])
    for target in (crowded, room["map"]):
        reg = LoamRegister()
        reg.setTarget(target)
        tree = oracle.KdTree(target)
        g, o, _ = _check_linearize(reg, tree, few, T)
        assert (o["status"] != 1).all()
        np.testing.assert_array_equal(g["nn"], o["nn"])
        _check_linearize(reg, tree, room["scan"], T)


def test_degenerate_and_failing_planes(gpu):
    """Five collinear neighbours, five coplanar ones on an exact lattice (rank-deficient fit: fewer than three non-zero
    pivots) and five that lie on no plane (failing plane gate): status and rows as the oracle's."""
    rng = np.random.default_rng(9)
    line = np.stack([np.arange(1200) * 0.05, np.zeros(1200), np.zeros(1200)], axis=1)                    # y = z = 0
    flat = _lattice(40, 40, 0.25, 0.0, 0.0, 20.0)                                                          # z = 0, exact
    skew = np.stack([np.arange(400) * 0.1, 40.0 + np.arange(400) * 0.1, np.arange(400) * 0.05], axis=1)  # a line off the axes
    blob = np.array([30.0, 60.0, 5.0]) + rng.uniform(-3, 3, (1800, 3))                                     # no plane anywhere
    m = _cloud(np.concatenate([line, flat, skew, blob]))
    q = np.concatenate([
        np.stack([rng.uniform(5, 55, 75), rng.normal(0, 0.02, 75), rng.normal(0, 0.02, 75)], axis=1),
        np.stack([rng.uniform(2, 8, 75), 20.0 + rng.uniform(2, 8, 75), rng.uniform(0.01, 0.3, 75)], axis=1),
        np.stack([(t := rng.uniform(5, 35, 75)), 40.0 + t, 0.5 * t + rng.normal(0, 0.02, 75)], axis=1),
        np.array([30.0, 60.0, 5.0]) + rng.uniform(-2.5, 2.5, (75, 3)),
    ])
    scan = _cloud(q[rng.permutation(300)])
    reg = LoamRegister()
    reg.setTarget(m)
    g, o, _ = _check_linearize(reg, oracle.KdTree(m), scan, np.eye(4))
    assert (o["status"] == 2).sum() >= 20, np.bincount(o["status"], minlength=5)      # the plane gate really fails somewhere
    assert np.isfinite(g["rows"]).all()


def test_fewer_than_five_neighbours(gpu, room):
    """Queries beyond the map's edge: some slots of the eight stay empty, fewer than five neighbours lie inside the gate --
    status 1 and rows of zeros, never a NaN."""
    rng = np.random.default_rng(4)
    T = room["truth"]
    out = np.stack([rng.uniform(-7.2, -6.3, 150), rng.uniform(-7.2, 5.0, 150), rng.uniform(-0.9, 0.9, 150)], axis=1)
    far = np.stack([rng.uniform(-40, -20, 50), rng.uniform(-40, 40, 50), rng.uniform(-5, 5, 50)], axis=1)
    scan = np.concatenate([room["scan"][:100], _cloud((np.concatenate([out, far]) - T[:3, 3]) @ T[:3, :3])])
    reg = LoamRegister()
    reg.setTarget(room["map"])
    g, o, _ = _check_linearize(reg, oracle.KdTree(room["map"]), scan, T)
    assert (o["status"][100:] == 1).sum() >= 100
    assert np.isfinite(g["rows"]).all()
    assert (g["rows"][g["status"] != 0] == 0).all()


def test_entries_written_late_are_complete(gpu, room):
    """The cache entries leave a block after its accumulate phase.  The next launch must still find every one complete: the same
    call twice on one handle (the second starts on the entries the first left) and once on a fresh handle, bit-equal poses."""
    T0 = synth.perturb(room["truth"], 3, trans=0.1, rot_deg=1.0)
    a, b = LoamRegister(loam_iters=10, loam_early_exit=0), LoamRegister(loam_iters=10, loam_early_exit=0)
    p1, p2, p3 = T0.copy(), T0.copy(), T0.copy()
    a.scan2Map(room["scan"], room["map"], p1)
    a.scan2Map(room["scan"], room["map"], p2)
    b.scan2Map(room["scan"], room["map"], p3)
    np.testing.assert_array_equal(p1, p2)
    np.testing.assert_array_equal(p1, p3)
    po, _, _ = oracle.loam_scan2map(room["scan"], room["map"], T0, oracle.loam_params(iters=10, early_exit=0))
    dt, dr = synth.pose_error(p1, po)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dt, dr)
