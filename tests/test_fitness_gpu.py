"""The fitness score's 1-NN search (vgicp.hip: fitness_kernel) against brute force, on every kind of index a handle may hold when it is asked:
a full grid at the three cell sizes (LOAM 1 m, NDT ndt_resolution, VGICP vgicp_resolution), a region-only lattice (from a handle's second
scan2Map on), an index cut to the bulk of the cloud or around a scan (header.clamped).

The device transforms the source in float in the reference's order and sums the squared distance in the order of the oracle's
sqdist_f32, so every per-point distance is bit for bit the brute-force float value (tests/fitness_ref.py): a single source point's score
equals its distance exactly, the count of a gate is exact, and a whole cloud's score differs only by the order of the double sum.  Against
an index that does not hold every target point the answer is the reference's number or a refusal that names the cut -- never another number.
"""
import numpy as np
import pytest

import fitness_ref as fr
import oracle
from simpleslam_amd import LoamRegister, NdtRegister, VgicpRegister, synth
from simpleslam_amd.pcr import PcrError

pytestmark = pytest.mark.gpu

DBL_MAX = fr.DBL_MAX
I4 = np.eye(4)

# name: (class, parameters, search cell of the index the score runs on)
HANDLES = {
    "loam": (LoamRegister, {}, 1.0),
    "ndt1": (NdtRegister, dict(ndt_resolution=1.0), 1.0),
    "ndt2": (NdtRegister, dict(ndt_resolution=2.0), 2.0),
    "vgicp1": (VgicpRegister, dict(vgicp_resolution=1.0), 1.0),
    "vgicp05": (VgicpRegister, dict(vgicp_resolution=0.5), 0.5),
}


def _rows(q, cols=4):
    a = np.zeros((len(q), cols), np.float32)
    a[:, :3] = np.asarray(q, np.float32).reshape(-1, 3)
    return a


def _last_error(reg):
    return reg._lib.pcr_last_error(reg._h).decode()


def _ref_knn(src, dst, pose):
    """per-point float squared distances of the whole source (the oracle's kd-tree, checked against brute force on the CPU)"""
    _, d2 = oracle.knn_f32(dst, fr.transform_f32(src, pose), 1)
    return d2[:, 0]


def _assert_score(got, d2, max_sq, what):
    want_s, want_n = fr.gated_from_sq(d2, max_sq)
    s, n = got
    assert n == want_n, (what, n, want_n)
    if want_n == 0:
        assert s == -1.0, (what, s)
    else:
        np.testing.assert_allclose(s, want_s, rtol=fr.sum_order_rtol(want_n), atol=0, err_msg=str(what))


def _until_region_only(reg, src, dst, inits, check=None):
    """scan2Map calls until the last one indexed the scan's region only (pcr_stats.region_index; possible from a handle's second call on, once
    an earlier full build's lattice can be taken over): the precondition of the tests below, asserted.  Returns the last pose."""
    for k, T0 in enumerate(inits):
        pose = T0.copy()
        c = reg.scan2Map(src, dst, pose)
        if check:
            check(T0, c, pose)
        if k >= 1 and reg.stats()["region_index"] == 1:
            break
    assert reg.stats()["region_index"] == 1
    return pose


def _probe(reg, target, queries, max_sq=DBL_MAX, what=""):
    """one source point per call: the score IS that point's float distance (or -1 with nothing counted)"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    d2, _ = fr.nearest_sq(q, target)
    for i in range(len(q)):
        got = reg.fitnessGated(_rows(q[i:i + 1]), I4, max_sq)
        d = np.float64(d2[i])
        want = (float(d), 1) if d <= max_sq else (-1.0, 0)
        assert got == want, (what, i, q[i].tolist(), got, want)


@pytest.fixture(scope="module")
def probe_world():
    world, m = synth.make_map(40_000, seed=31)
    scan, T = synth.make_scan(world, 0, seed=31, beams=16, azimuths=512)
    pts = m[:, :3]
    c = np.median(pts, axis=0).astype(np.float32)
    c[2] = np.float32(1.0)
    m = m[np.linalg.norm(pts - c, axis=1) > 6.0]                       # a cavity: nothing within 6 m of c (3 rings and more at every cell size)
    vals = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.25, -0.75, 1.5, -4.0], np.float32)
    on_faces = np.zeros((24, 4), np.float32)                           # target points on cell faces of every lattice (k cell and (k + 1/2) cell)
    for i in range(24):
        on_faces[i, :3] = [vals[i % 12], vals[(5 * i + 1) % 12], vals[(7 * i + 2) % 12]]
    m = np.ascontiguousarray(np.vstack([m, on_faces]), np.float32)
    lo, hi = m[:, :3].min(axis=0), m[:, :3].max(axis=0)
    return dict(map=m, scan=scan, truth=T, init=synth.perturb(T, 31, trans=0.2, rot_deg=1.0), cavity=c, lo=lo, hi=hi, vals=vals)


def _probe_queries(w, cell):
    m, lo, hi = w["map"], w["lo"], w["hi"]
    q = [m[k, :3] + np.float32([0.1, 0.05, -0.03]) for k in (17, 9000, 31000)]       # in occupied cells
    q += [w["cavity"], w["cavity"] + np.float32([1.0, -0.5, 0.25])]                     # empty region, nearest point 6 m away
    vals = w["vals"]
    q += [np.float32([vals[i], vals[(3 * i + 4) % 12], vals[(11 * i + 7) % 12]]) for i in range(12)]      # on cell faces, +-0
    q += [np.float32([0.0, -0.0, 0.0]), np.float32([-0.0, -0.0, -0.0])]
    mid = (lo + hi) / 2
    for delta in (0.5 * cell, 10.0, 1.0e4):                               # outside the grid box: beyond every face and a corner
        for d in range(3):
            for side in (-1, 1):
                p = mid.copy(); p[d] = (hi[d] + delta) if side > 0 else (lo[d] - delta)
                q.append(p)
        q.append(hi + np.float32(delta))
    return np.array(q, np.float32)


@pytest.mark.parametrize("name", list(HANDLES))
def test_single_point_probes(gpu, probe_world, name):
    """after setTarget and after two scan2Map calls (an NDT handle whose last call indexed the scan's region only indexes the staged copy again)"""
    cls, kw, cell = HANDLES[name]
    w = probe_world
    reg = cls(**kw)
    reg.setTarget(w["map"])
    queries = _probe_queries(w, cell)
    _probe(reg, w["map"], queries, what=(name, "setTarget"))
    for _ in range(2):
        pose = w["init"].copy()
        reg.scan2Map(w["scan"], w["map"], pose)
    _probe(reg, w["map"], queries, what=(name, "scan2Map"))
    # the gate at a float distance that occurs: d2 is counted, the double below it is not, the one above it is
    q = w["map"][9000:9001, :3] + np.float32([0.3, 0.2, 0.1])
    d2 = float(fr.nearest_sq(q, w["map"])[0][0])
    for g, n in ((d2, 1), (float(np.nextafter(d2, 0.0)), 0), (float(np.nextafter(d2, np.inf)), 1), (float(np.float32(d2)) * (1 - 1e-12), 0)):
        assert reg.fitnessGated(_rows(q), I4, g) == ((d2, 1) if n else (-1.0, 0)), (name, g)
    # source rows that are not finite: no distance, left out (oracle.fitness_score leaves them out too)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 1.0, 2.0], [1.0, 2.0, np.nan]], np.float32)
    for i in range(len(bad)):
        assert reg.fitnessGated(_rows(bad[i:i + 1]), I4, DBL_MAX) == (-1.0, 0), (name, bad[i])
    mixed = np.vstack([_rows(bad), _rows(queries[:3])])
    d = fr.nearest_sq(queries[:3], w["map"])[0]
    _assert_score(reg.fitnessGated(mixed, I4, DBL_MAX), d, DBL_MAX, (name, "mixed"))
    assert oracle.fitness_score(mixed, w["map"], I4) == pytest.approx(fr.gated_from_sq(d, DBL_MAX)[0], rel=fr.sum_order_rtol(3))


@pytest.mark.parametrize("name", list(HANDLES))
def test_tiny_and_unclean_targets(gpu, probe_world, name):
    """a target of one point, a target in one cell, a target with NaN and inf rows"""
    cls, kw, cell = HANDLES[name]
    w = probe_world
    rng = np.random.default_rng(8)
    one = _rows([[1.3, -0.7, 0.2]])
    clump = _rows(rng.uniform(0.26, 0.49, (50, 3)))                       # one cell of every lattice here (faces at k cell and (k + 1/2) cell)
    unclean = w["map"][::4].copy()
    unclean[::37, 0] = np.nan; unclean[5::41, 1] = np.inf; unclean[9::43, 2] = -np.inf
    q_small = np.float32([[1.3, -0.7, 0.2], [0.0, 0.0, 0.0], [0.3, 0.3, 0.3], [5.0, -3.0, 1.0], [-1.0e4, 2.0, 0.5], [0.49, 0.26, 0.375]])
    for tname, tgt, queries in (("one point", one, q_small), ("one cell", clump, q_small), ("NaN / inf rows", unclean, _probe_queries(w, cell)[:24])):
        reg = cls(**kw)
        reg.setTarget(tgt)
        _probe(reg, tgt, queries, what=(name, tname))


@pytest.mark.parametrize("name", ["loam", "vgicp1", "ndt2"])
def test_whole_clouds(gpu, probe_world, name):
    """n_src 0, 1, 255, 256, 257 and 131 073 (past 512 blocks of 256 threads: the kernel's grid-stride loop), 16- and 32-byte points,
    host and device sources, a gate and none: the count exact, the score within the bound of another summation order"""
    import torch
    cls, kw, _ = HANDLES[name]
    w = probe_world
    reg = cls(**kw)
    reg.setTarget(w["map"])
    rng = np.random.default_rng(11)
    lo, hi = w["lo"], w["hi"]
    src8 = np.zeros((131_073, 8), np.float32)
    src8[:, :3] = rng.uniform(lo - 5.0, hi + 5.0, (131_073, 3))
    src8[:, 3:] = rng.normal(0, 100, (131_073, 5))                       # (columns past xyz are not read)
    pose = synth.perturb(I4, 5, trans=0.5, rot_deg=3.0)
    d2 = _ref_knn(src8, w["map"], pose)
    for n in (0, 1, 255, 256, 257, 131_073):
        for cols in (4, 8):
            src = np.ascontiguousarray(src8[:n, :cols])
            for dev in (False, True):
                s = torch.from_numpy(src).cuda() if dev else src
                for gate in (1.0, DBL_MAX):
                    got = reg.fitnessGated(s, pose, gate)
                    if n == 0:
                        assert got == (-1.0, 0)
                    _assert_score(got, d2[:n], gate, (name, n, cols, dev, gate))


def test_baseline_sized_vgicp_handle(gpu):
    """65 536 points against 1 M, 0.5 m voxels, one handle through several calls (a region-only lattice from the second on): getFitnessScore
    and fitnessGated on every call against the reference, not against another handle"""
    world, m = synth.make_map(1_000_000, seed=41)
    reg = VgicpRegister(vgicp_resolution=0.5)
    for k in range(3):
        scan, T = synth.make_scan(world, k, seed=41)
        assert scan.shape[0] == 65_536
        pose = synth.perturb(T, 41 + k, trans=0.2, rot_deg=1.0)
        reg.scan2Map(scan, m, pose)
        if k > 0:
            assert reg.stats()["region_index"] == 1, k
        d2 = _ref_knn(scan, m, pose)
        got = reg.getFitnessScore()
        want, n = fr.gated_from_sq(d2, DBL_MAX)
        assert n == len(scan)
        np.testing.assert_allclose(got, want, rtol=fr.sum_order_rtol(n), atol=0, err_msg=str(k))
        np.testing.assert_allclose(got, oracle.fitness_score(scan, m, pose), rtol=fr.sum_order_rtol(n), atol=0)
        _assert_score(reg.fitnessGated(scan, pose, 1.0), d2, 1.0, k)
        off = synth.perturb(pose, 50 + k, trans=0.5, rot_deg=2.0)
        _assert_score(reg.fitnessGated(scan, off, 0.05), _ref_knn(scan, m, off), 0.05, (k, "off"))


@pytest.fixture(scope="module")
def big_world():
    world, m = synth.make_map(400_000, seed=77)
    scan, T = synth.make_scan(world, 1, seed=77)
    return dict(map=m, scan=scan, truth=T)


@pytest.mark.parametrize("on_device", [False, True])
def test_vgicp_gated_fitness_on_a_region_only_lattice(gpu, big_world, on_device):
    """A map-sized target (> 300 000 points) from a handle's second scan2Map on: the voxel lattice holds the scan's region only
    (region_index = 1); the score is searched on the covariance search grid, which holds every point -- host and device targets alike."""
    import torch
    w = big_world
    scan, m = w["scan"], w["map"]
    s_in, m_in = (torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda()) if on_device else (scan, m)
    reg = VgicpRegister()
    pose = _until_region_only(reg, s_in, m_in, [synth.perturb(w["truth"], 90 + k, trans=0.2, rot_deg=1.0) for k in range(4)])
    d2 = _ref_knn(scan, m, pose)
    _assert_score(reg.fitnessGated(s_in, pose, 1.0), d2, 1.0, "gated")
    np.testing.assert_allclose(reg.getFitnessScore(), fr.gated_from_sq(d2, DBL_MAX)[0], rtol=fr.sum_order_rtol(len(scan)), atol=0)
    off = synth.perturb(pose, 7, trans=1.0, rot_deg=5.0)
    _assert_score(reg.fitnessGated(s_in, off, 0.5), _ref_knn(scan, m, off), 0.5, "off")


def test_ndt_region_only_index_of_a_host_target(gpu, probe_world):
    """scan2Map x2 -> fitnessGated -> align -> scan2Map -> fitnessGated on one NDT handle: the score indexes the staged host copy again
    (replacing the handle's grid); every score is the reference's, every pose a fresh handle's bit for bit"""
    w = probe_world
    scan, m = w["scan"], w["map"]
    reg = NdtRegister()
    inits = [synth.perturb(w["truth"], 60 + k, trans=0.2, rot_deg=1.0) for k in range(6)]

    def fresh_scan2map(T0):
        p = T0.copy()
        c = NdtRegister().scan2Map(scan, m, p)
        return c, p

    def same_as_fresh(T0, c, p):
        cf, pf = fresh_scan2map(T0)
        assert c == cf
        np.testing.assert_array_equal(p, pf)

    p = _until_region_only(reg, scan, m, inits[:4], same_as_fresh)
    _assert_score(reg.fitnessGated(scan, p, 1.0), _ref_knn(scan, m, p), 1.0, "after scan2Map")
    kept = NdtRegister(); kept.setTarget(m)
    pa, pk = inits[4].copy(), inits[4].copy()
    assert reg.align(scan, pa) == kept.align(scan, pk)
    np.testing.assert_array_equal(pa, pk)
    p = inits[5].copy()
    same_as_fresh(inits[5], reg.scan2Map(scan, m, p), p)
    _assert_score(reg.fitnessGated(scan, p, 1.0), _ref_knn(scan, m, p), 1.0, "after the last scan2Map")
    _assert_score(reg.fitnessGated(scan, pa, 0.1), _ref_knn(scan, m, pa), 0.1, "at the aligned pose")


def test_ndt_region_only_index_of_a_device_target_is_refused(gpu, probe_world):
    import torch
    w = probe_world
    d_scan, d_map = torch.from_numpy(w["scan"]).cuda(), torch.from_numpy(w["map"]).cuda()
    reg = NdtRegister()
    _until_region_only(reg, d_scan, d_map, [w["init"]] * 4)
    with pytest.raises(PcrError, match="region only"):
        reg.fitnessGated(d_scan, w["init"], 1.0)


# ---- indexes cut to a region ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def two_clusters():
    """the map plus a thinned copy 30 km / 20 km / 8 km away: too spread out for dense tables, so a target index is cut to the bulk"""
    world, m = synth.make_map(60_000, seed=21)
    scan, T = synth.make_scan(world, 0, seed=21, beams=32, azimuths=512)
    init = synth.perturb(T, 21, trans=0.3, rot_deg=2.0)
    off = np.array([30000.0, 20000.0, 8000.0], np.float32)
    far = m[::200].copy(); far[:, :3] += off
    both = np.ascontiguousarray(np.vstack([m, far]))
    there = init.copy(); there[:3, 3] += off
    return dict(map=m, both=both, scan=scan, init=init, there=there, off=off)


def _answer_or_cut(call, d2, max_sq, what):
    """the reference's number, or a refusal that names the cut; returns whether it answered"""
    try:
        got = call()
    except PcrError as e:
        assert "cut" in str(e), (what, str(e))
        return False
    _assert_score(got, d2, max_sq, what)
    return True


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_gated_fitness_against_a_target_cut_to_its_bulk(gpu, two_clusters, method):
    w = two_clusters
    reg = LoamRegister() if method == "loam" else VgicpRegister()
    reg.setTarget(w["both"])
    for where, T in (("bulk", w["init"]), ("far cluster", w["there"])):
        for gate in (1.0, DBL_MAX):
            d2 = _ref_knn(w["scan"], w["both"], T)
            assert fr.gated_from_sq(d2, gate)[1] > 0
            answered = _answer_or_cut(lambda: reg.fitnessGated(w["scan"], T, gate), d2, gate, (method, where, gate))
            if where == "bulk":
                assert answered, (method, gate)       # the scan lies well inside the part that is indexed


def test_vgicp_scan2map_in_the_far_cluster_then_fitness_elsewhere(gpu, two_clusters):
    """scan2Map in the far cluster cuts the target around the scan; the score of that scan, and a gated score at the bulk pose, are the
    reference's or refused"""
    w = two_clusters
    reg = VgicpRegister()
    pose = w["there"].copy()
    reg.scan2Map(w["scan"], w["both"], pose)
    d2 = _ref_knn(w["scan"], w["both"], pose)
    got = reg.getFitnessScore()
    if got == -1.0:
        assert "cut" in _last_error(reg), _last_error(reg)
    else:
        np.testing.assert_allclose(got, fr.gated_from_sq(d2, DBL_MAX)[0], rtol=fr.sum_order_rtol(len(d2)), atol=0)
    for gate in (1.0, DBL_MAX):
        d2b = _ref_knn(w["scan"], w["both"], w["init"])
        _answer_or_cut(lambda: reg.fitnessGated(w["scan"], w["init"], gate), d2b, gate, ("bulk pose", gate))


def _bulk_box(cloud):
    """the region set_clamp_from_target_sample cuts a target to: per axis the 2nd and 98th percentile of a strided sample of <= 4096 points,
    widened by half their span + 20 m"""
    n = len(cloud)
    step = max(1, n // 4096)
    s = cloud[::step, :3].astype(np.float64)
    s = s[np.isfinite(s).all(axis=1)]
    lo, hi = np.zeros(3), np.zeros(3)
    for d in range(3):
        v = np.sort(s[:, d])
        a, b = v[int(0.02 * (len(v) - 1))], v[int(0.98 * (len(v) - 1) + 0.5)]
        pad = 0.5 * (b - a) + 20.0
        lo[d], hi[d] = a - pad, b + pad
    return lo, hi


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_nearest_target_point_beyond_a_cut_face(gpu, two_clusters, method):
    """a target point 40 m beyond the lower x face of the bulk box: a query just inside the box and one just beyond the face both have it as
    their nearest target point; the index left it out, so the answer is exact (found) or refused -- never the distance to the bulk"""
    w = two_clusters
    lo, hi = _bulk_box(w["both"])
    mid = (lo + hi) / 2
    stray = np.zeros((1, 4), np.float32)
    stray[0, :3] = [lo[0] - 40.0, mid[1], mid[2]]
    tgt = np.ascontiguousarray(np.vstack([w["both"], stray]))
    assert np.allclose(_bulk_box(tgt)[0], lo, atol=1.0)
    queries = np.float32([[lo[0] + 0.5, mid[1], mid[2]], [lo[0] - 38.0, mid[1] + 1.0, mid[2]], [lo[0] + 2.0, mid[1] - 3.0, mid[2] + 1.0]])
    d2, idx = fr.nearest_sq(queries, tgt)
    assert (idx == len(tgt) - 1).all(), idx                                 # the stray point is the nearest of every query
    reg = LoamRegister() if method == "loam" else VgicpRegister()
    reg.setTarget(tgt)
    for i in range(len(queries)):
        _answer_or_cut(lambda: reg.fitnessGated(_rows(queries[i:i + 1]), I4, DBL_MAX), d2[i:i + 1], DBL_MAX, (method, i))
    _answer_or_cut(lambda: reg.fitnessGated(_rows(queries), I4, DBL_MAX), d2, DBL_MAX, (method, "all"))
