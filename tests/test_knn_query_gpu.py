"""pcr_knn and pcr_radius_search (csrc/knn_query.hip) against the reference's nanoflann: its recorded answers (tests/golden), its code
compiled as it lies (oracle.ref_knn / ref_radius, when oracle/_ref is present) and the numpy restatement tests/knn_ref.py, which
tests/test_knn_ref.py pins to both.  Indices equal, squared distances bit for bit, no row left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import knn_ref
import oracle
from simpleslam_amd import LoamRegister, NdtRegister, VgicpRegister, synth
from simpleslam_amd.pcr import PcrError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def more():
    return np.load(os.path.join(G, "ref_nanoflann_more.npz"))


@pytest.fixture(scope="module")
def golden_reg(gpu, more):
    reg = LoamRegister()
    reg.setTarget(more["knn_points"])
    return reg


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    assert a.tobytes() == b.tobytes(), f"{int((a.view(np.uint64) != b.view(np.uint64)).sum())} of {a.size} distances differ in bits"


def _segments(off, idx):
    return [idx[int(off[j]):int(off[j + 1])] for j in range(len(off) - 1)]


def test_golden_k5(golden_reg, more):
    idx, d2 = golden_reg.knn(more["knn_queries"], 5)
    np.testing.assert_array_equal(idx, more["knn_idx"])
    _same_bits(d2, more["knn_d2"])


@pytest.mark.parametrize("k", [1, 5, 8, 20, 32])
def test_other_k(golden_reg, more, k):
    idx, d2 = golden_reg.knn(more["knn_queries"], k)
    want_i, want_d = knn_ref.knn(more["knn_points"], more["knn_queries"], k)
    print(f"k = {k}: {int((idx != want_i).any(axis=1).sum())} rows differ from knn_ref")
    np.testing.assert_array_equal(idx, want_i)
    _same_bits(d2, want_d)
    if oracle.ref_available():
        ref_i, ref_d = oracle.ref_knn(more["knn_points"], more["knn_queries"], k)
        np.testing.assert_array_equal(idx, ref_i)
        _same_bits(d2, ref_d)


@pytest.mark.parametrize("r", [0.5, 2.0])
def test_radius(golden_reg, more, r):
    q = more["knn_queries"][:256]
    off, idx, d2 = golden_reg.radiusSearch(q, r, sorted=True)
    w_off, w_idx, w_d2 = knn_ref.radius_search(more["knn_points"], q, r, sorted_=True)
    cnt = np.diff(off.astype(np.int64))
    print(f"r = {r}: {cnt.min()} .. {cnt.max()} neighbours per query, {len(idx)} in all")
    np.testing.assert_array_equal(off, w_off)
    np.testing.assert_array_equal(idx, w_idx)
    _same_bits(d2, w_d2)
    if oracle.ref_available():
        for j in range(len(q)):
            ri, rd = oracle.ref_radius(more["knn_points"], q[j, :3].astype(np.float64), r, sorted_=True)
            a, b = int(off[j]), int(off[j + 1])
            np.testing.assert_array_equal(idx[a:b], ri, err_msg=str(j))
            _same_bits(d2[a:b], rd)
    u_off, u_idx, u_d2 = golden_reg.radiusSearch(q, r, sorted=False)
    np.testing.assert_array_equal(u_off, off)
    for a, b in zip(_segments(off, idx), _segments(u_off, u_idx)):
        np.testing.assert_array_equal(np.sort(b), np.sort(a))
    o = np.lexsort((u_idx, np.repeat(np.arange(len(q)), cnt)))      # by query, then index: the distances travel with their points
    o_s = np.lexsort((idx, np.repeat(np.arange(len(q)), cnt)))
    _same_bits(u_d2[o], d2[o_s])


def test_radius_is_strict(gpu):
    reg = LoamRegister()
    reg.setTarget(np.array([[0, 0, 0, 0], [2, 0, 0, 0]], np.float32))
    q = np.zeros((1, 4), np.float32)
    off, idx, d2 = reg.radiusSearch(q, 2.0)
    np.testing.assert_array_equal(off, [0, 1]); np.testing.assert_array_equal(idx, [0])
    off, idx, d2 = reg.radiusSearch(q, float(np.nextafter(2.0, np.inf)))
    np.testing.assert_array_equal(off, [0, 2]); np.testing.assert_array_equal(idx, [0, 1]); np.testing.assert_array_equal(d2, [0.0, 4.0])


def test_sizing_in_two_calls(golden_reg, more):
    q = np.ascontiguousarray(more["knn_queries"][:64])
    off, idx, d2 = golden_reg.radiusSearch(q, 2.0)
    total = len(idx)
    assert total > 64
    lib, h = golden_reg._lib, golden_reg._h
    o2 = np.zeros(65, np.uint64); i2 = np.full(total, -7, np.int64); dd2 = np.zeros(total); n_total = C.c_size_t(0)
    op, ip, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    args = lambda cap: (h, q.ctypes.data_as(C.c_void_p), 64, 16, 0, 2.0, 1, cap, o2.ctypes.data_as(op), i2.ctypes.data_as(ip), dd2.ctypes.data_as(dp), C.byref(n_total))
    assert lib.pcr_radius_search(*args(total - 1)) != 0
    msg = lib.pcr_last_error(h).decode()
    assert str(total) in msg and str(total - 1) in msg, msg
    assert n_total.value == total
    np.testing.assert_array_equal(o2, off)
    assert lib.pcr_radius_search(*args(total)) == 0
    np.testing.assert_array_equal(o2, off); np.testing.assert_array_equal(i2, idx); _same_bits(dd2, d2)


def test_queries_far_outside_the_box(golden_reg, more):
    """500 m outside: the centre cell is clamped into the grid, so the termination bound has to come from the block scanned"""
    pts = more["knn_points"]
    lo, hi = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    mid = 0.5 * (lo + hi)
    q = np.zeros((8, 4), np.float32)
    q[:, :3] = mid
    q[0, 0] = hi[0] + 500; q[1, 0] = lo[0] - 500; q[2, 1] = hi[1] + 500; q[3, 1] = lo[1] - 500
    q[4, 2] = hi[2] + 500; q[5, 2] = lo[2] - 500; q[6, :3] = hi + 500; q[7, :3] = lo - np.float32([500, 3, 0.5])
    for k in (1, 5, 32):
        idx, d2 = golden_reg.knn(q, k)
        want_i, want_d = knn_ref.knn(pts, q, k)
        np.testing.assert_array_equal(idx, want_i)
        _same_bits(d2, want_d)
    off, idx, d2 = golden_reg.radiusSearch(q, 501.0)
    w_off, w_idx, w_d2 = knn_ref.radius_search(pts, q, 501.0)
    np.testing.assert_array_equal(off, w_off); np.testing.assert_array_equal(idx, w_idx); _same_bits(d2, w_d2)


def test_edge_cases(gpu):
    reg = LoamRegister()
    with pytest.raises(PcrError, match="no kept target"):
        reg.knn(np.zeros((1, 4), np.float32), 1)
    with pytest.raises(PcrError, match="no kept target"):
        reg.radiusSearch(np.zeros((1, 4), np.float32), 1.0)
    # fewer than k points, a duplicated point, target points that are not finite (they renumber nothing)
    pts = np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0], [2, 0, 0, 0], [0, np.inf, 0, 0], [2, 0, 0, 0], [5, 1, 0, 0]], np.float32)
    reg.setTarget(pts)
    q = np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0], [1.5, 0, 0, 0], [0, 0, -np.inf, 0]], np.float32)
    idx, d2 = reg.knn(q, 5)
    want_i, want_d = knn_ref.knn(pts, q, 5)
    np.testing.assert_array_equal(want_i[0], [0, 2, 4, 5, -1])
    np.testing.assert_array_equal(idx, want_i)
    _same_bits(d2, want_d)
    assert (idx[1] == -1).all() and np.isposinf(d2[1]).all() and (idx[3] == -1).all() and np.isposinf(d2[3]).all()
    off, ridx, rd2 = reg.radiusSearch(q, 3.0)
    w = knn_ref.radius_search(pts, q, 3.0)
    np.testing.assert_array_equal(off, w[0]); np.testing.assert_array_equal(ridx, w[1]); _same_bits(rd2, w[2])
    np.testing.assert_array_equal(off, [0, 3, 3, 6, 6])
    for k in (0, 33, -1):
        with pytest.raises(PcrError, match="PCR_KNN_MAX_K"):
            reg.knn(q, k)
    for r in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(PcrError, match="radius"):
            reg.radiusSearch(q, r)
    idx, d2 = reg.knn(np.zeros((0, 4), np.float32), 5)
    assert idx.shape == (0, 5) and d2.shape == (0, 5)
    off, ridx, rd2 = reg.radiusSearch(np.zeros((0, 4), np.float32), 1.0)
    np.testing.assert_array_equal(off, [0]); assert len(ridx) == 0 and len(rd2) == 0
    # a target with no finite point at all
    reg.setTarget(np.full((3, 4), np.nan, np.float32))
    idx, d2 = reg.knn(q, 2)
    assert (idx == -1).all() and np.isposinf(d2).all()
    assert reg.radiusSearch(q, 1.0)[0].tolist() == [0] * 5


def test_equivalent_inputs(golden_reg, more):
    import torch
    q16 = np.ascontiguousarray(more["knn_queries"][:512])
    q32 = np.zeros((512, 8), np.float32); q32[:, :4] = q16; q32[:, 4:] = 9.0
    base = golden_reg.knn(q16, 8)
    rbase = golden_reg.radiusSearch(q16, 0.75)
    for q in (q32, torch.from_numpy(q16).cuda(), torch.from_numpy(q32).cuda()):
        idx, d2 = golden_reg.knn(q, 8)
        np.testing.assert_array_equal(idx, base[0]); _same_bits(d2, base[1])
        r = golden_reg.radiusSearch(q, 0.75)
        for a, b in zip(r, rbase):
            np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def small_world():
    world, m = synth.make_map(30_000, seed=5)
    scan, T = synth.make_scan(world, 0, seed=5, beams=16, azimuths=512)
    return dict(map=m, scan=scan, truth=T, init=synth.perturb(T, 5, trans=0.2, rot_deg=1.0))


@pytest.mark.parametrize("cls", [LoamRegister, NdtRegister, VgicpRegister])
def test_every_methods_handle(gpu, small_world, cls):
    w = small_world
    q = np.ascontiguousarray(fitness_points(w)[:1024])
    want_i, want_d = knn_ref.knn(w["map"], q, 8)
    w_off, w_idx, w_d2 = knn_ref.radius_search(w["map"], q[:128], 1.5)
    reg = cls()
    reg.setTarget(w["map"])
    idx, d2 = reg.knn(q, 8)
    np.testing.assert_array_equal(idx, want_i); _same_bits(d2, want_d)
    off, ridx, rd2 = reg.radiusSearch(q[:128], 1.5)
    np.testing.assert_array_equal(off, w_off); np.testing.assert_array_equal(ridx, w_idx); _same_bits(rd2, w_d2)


def fitness_points(w):
    """the scan at its true pose, in float: queries that lie in the map"""
    T = w["truth"].astype(np.float32)
    p = w["scan"][:, :3]
    out = np.zeros((p.shape[0], 4), np.float32)
    out[:, :3] = p @ T[:3, :3].T + T[:3, 3]
    return out


@pytest.mark.parametrize("cls", [NdtRegister, VgicpRegister])
def test_full_cloud_behind_a_region_only_index(gpu, cls):
    """From a handle's second pcr_scan2map on a map-sized host target the lattice holds the scan's region only (pcr_stats.region_index);
    the queries still answer from every point -- far from the scan as well"""
    world, m = synth.make_map(400_000, seed=77)
    scan, T = synth.make_scan(world, 1, seed=77)
    reg = cls()
    region_index = 0
    for off in (0.2, -0.3, 0.1):
        p = T.copy(); p[:3, 3] += np.array([off, -0.5 * off, 0.03 * off])
        reg.scan2Map(scan, m, p)
        region_index += reg.stats()["region_index"]
    assert region_index >= 1
    rng = np.random.default_rng(3)
    q = np.ascontiguousarray(m[rng.choice(len(m), 192, replace=False)])      # all over the map
    q[:, :3] += rng.normal(0, 0.05, (192, 3)).astype(np.float32)
    want_i, want_d = knn_ref.knn(m, q, 5, chunk=32)
    idx, d2 = reg.knn(q, 5)
    np.testing.assert_array_equal(idx, want_i); _same_bits(d2, want_d)
    w_off, w_idx, w_d2 = knn_ref.radius_search(m, q[:64], 1.0, chunk=32)
    off, ridx, rd2 = reg.radiusSearch(q[:64], 1.0)
    np.testing.assert_array_equal(off, w_off); np.testing.assert_array_equal(ridx, w_idx); _same_bits(rd2, w_d2)
    # and the next registration is what it would have been
    other = cls()
    for off_ in (0.2, -0.3, 0.1):
        p = T.copy(); p[:3, 3] += np.array([off_, -0.5 * off_, 0.03 * off_])
        other.scan2Map(scan, m, p)
    pa = T.copy(); pa[0, 3] += 0.15; pb = pa.copy()
    assert reg.scan2Map(scan, m, pa) == other.scan2Map(scan, m, pb)
    np.testing.assert_array_equal(pa, pb)


@pytest.mark.parametrize("cls", [LoamRegister, NdtRegister, VgicpRegister])
def test_no_side_effects_on_align(gpu, small_world, cls):
    w = small_world
    reg = cls()
    reg.setTarget(w["map"])
    p0 = w["init"].copy(); c0 = reg.align(w["scan"], p0)
    q = fitness_points(w)[:2048]
    reg.knn(q, 20); reg.radiusSearch(q[:256], 1.0); reg.radiusSearch(q[:256], 1.0, sorted=False)
    p1 = w["init"].copy(); c1 = reg.align(w["scan"], p1)
    assert c0 == c1
    np.testing.assert_array_equal(p0, p1)
    fresh = cls(); fresh.setTarget(w["map"])
    p2 = w["init"].copy(); fresh.align(w["scan"], p2)
    np.testing.assert_array_equal(p0, p2)


def test_kdtree_bench_prints_the_query_lines(gpu, small_world, tmp_path):
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "kdtree_bench")
    assert os.path.exists(exe), "kdtree_bench not built (run __graft_entry__.build())"
    w = small_world
    w["map"].astype(np.float32).tofile(tmp_path / "map.f32")
    fitness_points(w).tofile(tmp_path / "queries.f32")
    out = subprocess.run([exe, str(tmp_path / "map.f32"), str(tmp_path / "queries.f32"), "5", "5", "2.0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 4, out.stdout
    nq = w["scan"].shape[0]
    assert lines[2].startswith("pcr_knn k = 5:") and f"{nq} queries" in lines[2] and float(lines[2].split()[-2]) > 0
    assert lines[3].startswith("pcr_radius_search r = 2") and f"{nq} queries" in lines[3]
    words = lines[3].split()
    assert float(words[words.index("ns/query,") - 1]) > 0 and float(words[-1]) > 0      # ns/query and the mean count
