"""The sparse target index on the device (csrc/sparse_index.hip; pcr_params.query_index): pcr_knn and pcr_radius_search on targets whose box no
dense cell table holds -- two clusters 30 km apart, a stray return at 4e6 m -- and, under query_index = SPARSE, on ordinary ones.  Every answer
against brute force (knn_ref.py): indices equal, squared distances bit for bit; and SPARSE against AUTO (the dense index) byte for byte.
tests/test_sparse_index_host.py holds the same walk to its look-up bound on the CPU and runs first."""
import os
import subprocess

import numpy as np
import pytest

import knn_ref
import sparse_index_cases as cases
from simpleslam_amd import LoamRegister, VgicpRegister
from simpleslam_amd.pcr import QUERY_INDEX_SPARSE, PcrError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
KS = (1, 8, 9, 32)
RADII = (0.5, 3.0, 40000.0)


@pytest.fixture(scope="module", autouse=True)
def walk_is_bounded_on_the_cpu(tmp_path_factory):
    """No test of this file runs a kernel before the walk the kernels compile (csrc/sparse_walk.h) has been held, on the CPU, to its look-up bound
    on the far queries of the two-cluster cloud: a walk whose cost grew with the empty space would hang a GPU.  (tests/test_sparse_index_host.py
    checks far more, in the CPU suite; the order of two suites is nobody's promise, so the guard stands here.)"""
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "sparse_index_check")
    assert os.path.exists(exe), "sparse_index_check not built (run __graft_entry__.build())"
    d = tmp_path_factory.mktemp("walk")
    t = cases.two_clusters()
    t.tofile(d / "t.f32"); cases.queries_for(t, seed=11).tofile(d / "q.f32")
    out = subprocess.run([exe, str(d / "t.f32"), str(d / "q.f32"), "32", "40000.0", str(d / "o.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-300:] + out.stderr
    for line in out.stdout.splitlines():
        if line.startswith("q "):
            w = line.split()
            c = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
            assert c["knn_lookups"] <= 102 + 1 + c["knn_box"] * (1 + 5 * c["knn_rows"] + 2 * c["knn_layers"]), line
            assert c["rad_lookups"] <= c["rad_box"] * (1 + 5 * c["rad_rows"] + 2 * c["rad_layers"]), line


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    assert a.tobytes() == b.tobytes(), f"{int((a.view(np.uint64) != b.view(np.uint64)).sum())} of {a.size} distances differ in bits"


def _check_knn(reg, target, q, ks=KS):
    for k in ks:
        idx, d2 = reg.knn(q, k)
        want_i, want_d = knn_ref.knn(target, q, k)
        np.testing.assert_array_equal(idx, want_i, err_msg=f"k = {k}")
        _same_bits(d2, want_d)


def _check_radius(reg, target, q, radii=RADII):
    for r in radii:
        w_off, w_idx, w_d2 = knn_ref.radius_search(target, q, r, sorted_=True)
        off, idx, d2 = reg.radiusSearch(q, r, sorted=True)
        np.testing.assert_array_equal(off, w_off, err_msg=f"r = {r}")
        np.testing.assert_array_equal(idx, w_idx)
        _same_bits(d2, w_d2)
        u_off, u_idx, u_d2 = reg.radiusSearch(q, r, sorted=False)
        np.testing.assert_array_equal(u_off, w_off)
        seg = np.repeat(np.arange(len(q)), np.diff(w_off.astype(np.int64)))
        o = np.lexsort((u_idx, seg))      # by query, then index: the distances travel with their points
        o_w = np.lexsort((w_idx, seg))
        np.testing.assert_array_equal(u_idx[o], w_idx[o_w])
        _same_bits(u_d2[o], w_d2[o_w])


@pytest.fixture(scope="module")
def spread(gpu):
    """the two targets the dense index cannot hold, each set once on a handle under the default AUTO"""
    out = {}
    for name, t in (("two_clusters", cases.two_clusters()), ("stray", cases.stray())):
        reg = LoamRegister()
        reg.setTarget(t)
        out[name] = (reg, t, cases.queries_for(t, seed=11))
    return out


@pytest.mark.parametrize("name", ["two_clusters", "stray"])
def test_auto_answers_where_the_dense_index_was_cut(spread, name):
    """under AUTO these targets were refused ("the target's box cannot be tabulated ... an exact query needs every point"); now every answer is exact:
    queries inside a cluster, halfway between the clusters, 15 km outside the box, rows that are not finite"""
    reg, t, q = spread[name]
    _check_knn(reg, t, q)
    info = reg.queryIndexInfo()
    assert info["kind"] == "sparse" and info["n_points"] == len(t) and info["bytes"] == 24 * len(t)
    _check_radius(reg, t, q)
    bad = ~np.isfinite(q[:, :3]).all(axis=1)
    idx, d2 = reg.knn(q, 8)
    assert bad.sum() == 3 and (idx[bad] == -1).all() and np.isposinf(d2[bad]).all()


def test_auto_on_a_vgicp_handle(gpu, cls=VgicpRegister):
    """(the other method that cuts such a target to its bulk; ndt, gicp and liorf refuse it when it is set)"""
    t = cases.two_clusters(n=200, seed=4)
    q = cases.queries_for(t, seed=2, n_in=8)
    reg = cls()
    reg.setTarget(t)
    _check_knn(reg, t, q, ks=(5,))
    assert reg.queryIndexInfo()["kind"] == "sparse"
    _check_radius(reg, t, q, radii=(3.0,))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_sizes_at_the_wave_tile_and_block_edges(gpu, n):
    """cell faces, negative coordinates, exact duplicates and exact ties (the lower index wins), a target row that is not finite, fewer points than k:
    SPARSE against brute force, and against AUTO (the dense index of the same cloud) byte for byte"""
    t = cases.edge_cloud(n, seed=n)
    if n > 2:
        t[n // 2, 1] = np.nan
    q = cases.queries_for(t, seed=n + 1, n_in=12)
    sp, de = LoamRegister(query_index=QUERY_INDEX_SPARSE), LoamRegister()
    sp.setTarget(t); de.setTarget(t)
    _check_knn(sp, t, q)
    _check_radius(sp, t, q)
    assert sp.queryIndexInfo() == dict(kind="sparse", n_points=n - (n > 2), bytes=24 * n)
    for k in KS:
        a, b = sp.knn(q, k), de.knn(q, k)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for r in RADII:
        a, b = sp.radiusSearch(q, r), de.radiusSearch(q, r)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert de.queryIndexInfo()["kind"] == "dense"


def test_sparse_equals_auto_on_the_nanoflann_golden_vectors(gpu):
    g = np.load(os.path.join(G, "knn_nanoflann.npz"))
    sp, de = LoamRegister(query_index=QUERY_INDEX_SPARSE), LoamRegister()
    sp.setTarget(g["points"]); de.setTarget(g["points"])
    idx, d2 = sp.knn(g["queries"], 5)
    _same_bits(d2, g["d2"])      # (the cloud holds exact duplicates: nanoflann's order among ties follows its tree walk, ours the index -- the dense index's, below)
    tied = (np.diff(g["d2"], axis=1) == 0).any(axis=1)
    np.testing.assert_array_equal(idx[~tied], g["idx"][~tied])
    for k in (1, 5, 20, 32):
        a, b = sp.knn(g["queries"], k), de.knn(g["queries"], k)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    a, b = sp.radiusSearch(g["queries"][:128], 1.0), de.radiusSearch(g["queries"][:128], 1.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[1]) > 128
    assert (sp.queryIndexInfo()["kind"], de.queryIndexInfo()["kind"]) == ("sparse", "dense")


def test_the_byte_count_does_not_depend_on_the_box(spread):
    reg, t, _ = spread["two_clusters"]
    near = LoamRegister(query_index=QUERY_INDEX_SPARSE)
    near.setTarget(cases.two_clusters(gap=(30.0, 20.0, 8.0)))
    assert near.queryIndexInfo()["kind"] is None      # nothing has answered yet
    near.knn(t[:4], 1)
    reg.knn(t[:4], 1)
    assert near.queryIndexInfo() == reg.queryIndexInfo() == dict(kind="sparse", n_points=600, bytes=24 * 600)


def test_a_new_target_drops_the_index_and_the_setting_can_change(gpu):
    a, b = cases.two_clusters(n=100, seed=7), cases.stray(n=150, seed=8)
    q = cases.queries_for(a, seed=3, n_in=6)
    reg = LoamRegister()
    reg.setTarget(a)
    _check_knn(reg, a, q, ks=(8,))
    reg.setTarget(b)
    assert reg.queryIndexInfo()["kind"] is None
    _check_knn(reg, b, q, ks=(8,))
    assert reg.queryIndexInfo() == dict(kind="sparse", n_points=150, bytes=24 * 150)
    dense = cases.edge_cloud(500, seed=1)
    # a compact target on the handle that held a cut one: its index may take over the cut box as a hint, and with it the mark of the cut, so AUTO may
    # answer it from either index (include/pcr_hip.h says so) -- exactly either way
    reg.setTarget(dense)
    _check_knn(reg, dense, q, ks=(8,))
    assert reg.queryIndexInfo()["kind"] in ("dense", "sparse")
    reg = LoamRegister()      # a fresh handle: the dense index
    reg.setTarget(dense)
    _check_knn(reg, dense, q, ks=(8,))
    assert reg.queryIndexInfo()["kind"] == "dense"
    reg.set_params(query_index=QUERY_INDEX_SPARSE)
    _check_knn(reg, dense, q, ks=(8,))
    assert reg.queryIndexInfo()["kind"] == "sparse"
    with pytest.raises(PcrError, match="query_index"):
        reg.set_params(query_index=2)
    reg.invalidateTarget()
    with pytest.raises(PcrError, match="no kept target"):
        reg.knn(q, 1)


def test_a_callers_device_target_is_refused_by_the_sparse_index(gpu):
    """pcr_scan2map_device leaves the target in the caller's buffer, which may be gone by the time of a query: the dense index holds its own sorted
    copy and answers, the sparse index has nothing of its own to be built from and says so; setTarget (which copies) serves both"""
    import torch
    from simpleslam_amd import synth
    world, m = synth.make_map(20_000, seed=5)
    scan, T = synth.make_scan(world, 0, seed=5, beams=16, azimuths=256)
    reg = LoamRegister()
    pose = T.copy()
    reg.scan2Map(torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda(), pose)
    q = np.ascontiguousarray(m[:64])
    reg.knn(q, 5)
    assert reg.queryIndexInfo()["kind"] == "dense"
    reg.set_params(query_index=QUERY_INDEX_SPARSE)
    with pytest.raises(PcrError, match="device buffer of the caller's"):
        reg.knn(q, 5)
    with pytest.raises(PcrError, match="pcr_set_target"):
        reg.radiusSearch(q, 1.0)
    reg.setTarget(torch.from_numpy(m).cuda())      # (copied: the handle's own from now on)
    _check_knn(reg, m, q, ks=(5,))
    assert reg.queryIndexInfo()["kind"] == "sparse"
    pose = T.copy()
    reg.scan2Map(scan, m, pose)                     # a host target lies in the handle's staging area
    _check_knn(reg, m, q, ks=(5,))
    assert reg.queryIndexInfo()["kind"] == "sparse"


def test_a_stray_point_at_3e38_m_is_refused_and_the_handle_stays_usable(gpu):
    t = cases.stray(at=3.0e38)
    reg = LoamRegister()
    reg.setTarget(t)
    with pytest.raises(PcrError, match=r"extents 3e\+38 x \S+ x 3e\+38 cells"):
        reg.knn(t[:4], 1)
    with pytest.raises(PcrError, match=r"extents 3e\+38"):
        reg.radiusSearch(t[:4], 1.0)
    good = cases.stray()
    reg.setTarget(good)
    _check_knn(reg, good, cases.queries_for(good, seed=1, n_in=6), ks=(9,))


def test_kdtree_bench_sparse_agrees_with_the_binding(gpu, tmp_path):
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "kdtree_bench")
    assert os.path.exists(exe), "kdtree_bench not built (run __graft_entry__.build())"
    t = cases.edge_cloud(2049, seed=6)
    q = np.ascontiguousarray(cases.queries_for(t, seed=9)[:30])      # (the finite ones)
    t.tofile(tmp_path / "map.f32"); q.tofile(tmp_path / "queries.f32")
    out = subprocess.run([exe, str(tmp_path / "map.f32"), str(tmp_path / "queries.f32"), "2", "5", "2.0", "sparse"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 5 and lines[2].startswith("pcr_knn k = 5:") and lines[4].startswith("query index: sparse, 2049 points, 49176 bytes"), out.stdout
    reg = LoamRegister(query_index=QUERY_INDEX_SPARSE)
    reg.setTarget(t)
    off, idx, d2 = reg.radiusSearch(q, 2.0)
    assert int(lines[4].split()[-1]) == int(idx.sum())
    assert abs(float(lines[3].split()[-1]) - len(idx) / len(q)) < 0.006
