"""pcr_knn and pcr_radius_search (csrc/knn_query.hip, csrc/query_host.hip) where tests/test_knn_query_gpu.py does not reach: every kernel
instantiation and every k at a switch, exact distance ties, points and queries within two ulps of a cell face on the three lattices, radius
segments around the fill's 64, the sort's 256 and its 1024-key tiles, counts across the scan's 1024-count chunks, the host's 2^20-query
chunks.  The inputs are tests/knn_cases.py (held to their conditions by tests/test_knn_cases.py), the reference is tests/knn_ref.py, and
every comparison is exact: indices and offsets equal, squared distances equal in bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_cases
import knn_ref
import oracle
from simpleslam_amd import LoamRegister, NdtRegister, VgicpRegister

pytestmark = pytest.mark.gpu

HANDLES = {"loam": LoamRegister, "ndt": NdtRegister, "vgicp": VgicpRegister}


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    assert a.tobytes() == b.tobytes(), f"{int((a.view(np.uint64) != b.view(np.uint64)).sum())} of {a.size} distances differ in bits"


def _same_knn(got, want_i, want_d, what=""):
    idx, d2 = got
    bad = np.flatnonzero((idx != want_i).any(axis=1) | (d2.view(np.uint64) != want_d.view(np.uint64)).any(axis=1))
    if len(bad):
        j = int(bad[0])
        print(f"{what}: {len(bad)} of {len(idx)} rows differ; row {j}: got {idx[j].tolist()} {d2[j].tolist()}, want {want_i[j].tolist()} {want_d[j].tolist()}")
    np.testing.assert_array_equal(idx, want_i, err_msg=what)
    _same_bits(d2, want_d)


def _same_radius(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    _same_bits(got[2], want[2])


def _same_sets(got, want):
    """unsorted segments: the offsets equal, the same indices per query, every distance with its index"""
    np.testing.assert_array_equal(got[0], want[0])
    seg = np.repeat(np.arange(len(got[0]) - 1), np.diff(got[0].astype(np.int64)))
    o_g, o_w = np.lexsort((got[1], seg)), np.lexsort((want[1], seg))
    np.testing.assert_array_equal(got[1][o_g], want[1][o_w])
    _same_bits(got[2][o_g], want[2][o_w])


# ---- 1 - 3: every kernel, every k edge, nothing past k columns, fewer points than k ---------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    target = knn_cases.random_cloud(4000, seed=41)
    q = knn_cases.random_queries(321, target, seed=43)      # 256 + 65: a partial last block for blocks of 256 and of 64
    rng = np.random.default_rng(44)
    q[300:, :3] = rng.uniform(-40, 40, (21, 3)).astype(np.float32)      # some well outside the box: rings to the grid's edge
    want = knn_ref.knn(target, q, 32)      # the first k columns are the answer for k
    return dict(target=target, q=q, want=want)


@pytest.fixture(scope="module")
def cloud_reg(gpu, cloud):
    reg = LoamRegister()
    reg.setTarget(cloud["target"])
    return reg


@pytest.mark.parametrize("k", [1, 2, 7, 8, 9, 15, 16, 17, 31, 32])
def test_every_kernel_and_k_edge(cloud_reg, cloud, k):
    """knn_query_kernel<1,256> (k = 1), <8,256> (2 .. 8), <16,64> (9 .. 16), <32,64> (17 .. 32): each with k at and below its K"""
    _same_knn(cloud_reg.knn(cloud["q"], k), cloud["want"][0][:, :k], cloud["want"][1][:, :k], f"k = {k}")


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("k", [8, 16])
def test_query_counts_at_the_block_edges(cloud_reg, cloud, k, n_q):
    q = np.ascontiguousarray(cloud["q"][321 - n_q:])      # the far queries are in every one
    _same_knn(cloud_reg.knn(q, k), cloud["want"][0][321 - n_q:, :k], cloud["want"][1][321 - n_q:, :k], f"k = {k}, n_q = {n_q}")


@pytest.mark.parametrize("k", [2, 9, 17])
def test_nothing_is_written_past_k_columns(cloud_reg, cloud, k):
    """k one past a kernel switch, through the C ABI into arrays longer than n_q * k: the rows are right (a list written at its template
    length K would run over the next row) and the tail keeps its sentinel"""
    q, n, pad = cloud["q"], 321, 64
    idx = np.full(n * k + pad, -7, np.int64); d2 = np.full(n * k + pad, -3.0)
    rc = cloud_reg._lib.pcr_knn(cloud_reg._h, q.ctypes.data_as(C.c_void_p), n, 16, 0, k, idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, cloud_reg._lib.pcr_last_error(cloud_reg._h).decode()
    _same_knn((idx[:n * k].reshape(n, k), d2[:n * k].reshape(n, k)), cloud["want"][0][:, :k], cloud["want"][1][:, :k], f"k = {k}")
    assert (idx[n * k:] == -7).all() and (d2[n * k:] == -3.0).all()


@pytest.mark.parametrize("n_pts", [1, 7, 9, 17, 31])
def test_fewer_points_than_k(gpu, cloud, n_pts):
    target = np.ascontiguousarray(cloud["target"][:n_pts])
    q = np.ascontiguousarray(cloud["q"][:70]); q[5, 1] = np.nan
    reg = LoamRegister()
    reg.setTarget(target)
    for k in (8, 16, 32):
        want_i, want_d = knn_ref.knn(target, q, k)
        m = min(k, n_pts)
        assert (want_i[0, :m] >= 0).all() and (want_i[0, m:] == -1).all() and np.isposinf(want_d[0, m:]).all() and (want_i[5] == -1).all()
        _same_knn(reg.knn(q, k), want_i, want_d, f"{n_pts} points, k = {k}")


# ---- 4: exact ties ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice_case(which, copies):
    lat = knn_cases.lattices(copies)[which]
    return lat, knn_ref.knn(lat.target, lat.queries, 33)      # column k is the (k + 1)-th distance: whether the cut goes through a tie


def _whole_blocks_sorted(idx, d2, d_next):
    """idx with every block of equal distances in ascending index order, and -1 in the block the k-th place cuts (d2[k - 1] == d_next)"""
    cut = (d2 == d2[:, -1:]) & (d2[:, -1] == d_next)[:, None]
    a = np.where(cut, -1, idx)
    by_idx = np.argsort(a, axis=1, kind="stable")
    a, d = np.take_along_axis(a, by_idx, axis=1), np.take_along_axis(d2, by_idx, axis=1)
    return np.take_along_axis(a, np.argsort(d, axis=1, kind="stable"), axis=1)      # by distance, equal distances by index


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name", ["loam", "ndt", "vgicp"])
def test_ties(gpu, name, which, copies):
    """Equal distances everywhere: rows ascend by (d2, index), so the lower index wins the k-th place, whatever the order the index
    stores and visits the points in.  The lattice points lie on cell faces of at least one of the three lattices."""
    lat, (want_i, want_d) = _lattice_case(which, copies)
    reg = HANDLES[name]()
    reg.setTarget(lat.target)
    for k in lat.values:
        got = reg.knn(lat.queries, k)
        _same_knn(got, want_i[:, :k], want_d[:, :k], f"{name}, lattice {which} x {copies}, k = {k}")
        if oracle.ref_available():
            # nanoflann: the same distances; the same points in every block of equal distances that the k-th place does not cut (inside a
            # block, and in the one that is cut, its choice follows its tree walk and is not compared)
            ref_i, ref_d = oracle.ref_knn(lat.target, lat.queries, k)
            _same_bits(got[1], ref_d)
            np.testing.assert_array_equal(_whole_blocks_sorted(got[0], got[1], want_d[:, k]), _whole_blocks_sorted(ref_i, ref_d, want_d[:, k]))


# ---- 5: cell faces ------------------------------------------------------------------------------------------------------------------
def _face_handle(name):
    """The handle and its lattice (cell, shift), from its parameters.  loam: the smallest power of two >= sqrt(loam_knn_max_sq), not
    shifted.  vgicp: vgicp_resolution, shifted by half a cell.  ndt: float(ndt_resolution), not shifted, the cell index computed in float
    as pcl::VoxelGrid does -- at 0.7 m, since at the default 1 m float x * (1 / leaf) and f64 x / leaf cannot disagree."""
    if name == "loam":
        reg = LoamRegister()
        assert reg.params.loam_knn_max_sq == 1.0
        return reg, 1.0, 0.0
    if name == "vgicp":
        reg = VgicpRegister()
        assert reg.params.vgicp_resolution == 1.0
        return reg, 1.0, 0.5
    reg = NdtRegister(ndt_resolution=0.7)
    return reg, float(np.float32(reg.params.ndt_resolution)), 0.0


@pytest.mark.parametrize("centre", [knn_cases.NEAR, knn_cases.FAR], ids=["near", "far"])
@pytest.mark.parametrize("name", ["loam", "ndt", "vgicp"])
def test_faces(gpu, name, centre):
    """Target points and queries on the faces of the handle's own lattice and one and two ulps off them, around a few metres and around
    250 - 300 m: a point the build put into the cell next door, or a query whose centre cell is, must change nothing"""
    reg, cell, shift = _face_handle(name)
    fc = knn_cases.face_cloud(cell, shift, centre, seed=21, float_lattice=name == "ndt")
    reg.setTarget(fc.target)
    ks, radii = fc.values
    want_i, want_d = knn_ref.knn(fc.target, fc.queries, max(ks))
    for k in ks:
        _same_knn(reg.knn(fc.queries, k), want_i[:, :k], want_d[:, :k], f"{name} {centre}, k = {k}")
    for r in radii:
        want = knn_ref.radius_search(fc.target, fc.queries, r)
        assert want[0][-1] > len(fc.queries)
        _same_radius(reg.radiusSearch(fc.queries, r), want, f"{name} {centre}, r = {r}")
    for g in fc.slop_probes:      # (the float lattice: tests/test_knn_cases.py says why each of these needs the search's slop)
        q = np.ascontiguousarray(fc.queries[g.qrows])
        _same_radius(reg.radiusSearch(q, g.radius), knn_ref.radius_search(fc.target, q, g.radius), f"{name} {centre}, slop probe r = {g.radius}")


# ---- 6 - 8: radius search ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shell_case():
    return knn_cases.shells(2500, seed=31)


@pytest.fixture(scope="module")
def shell_reg(gpu, shell_case):
    reg = LoamRegister()
    reg.setTarget(shell_case.target)
    return reg


@pytest.mark.parametrize("m", knn_cases.SHELL_LENGTHS)
def test_radius_segment_lengths(shell_reg, shell_case, m):
    """segments of exactly m entries: around the 64 points a wave takes from a row at a time, the 256 entries a sort block ranks at a
    time and the 1024 keys of an LDS tile; all of one row of the index"""
    sh, r = shell_case, shell_case.radius(m)
    want = knn_ref.radius_search(sh.target, sh.queries, r, sorted_=True)
    np.testing.assert_array_equal(want[0], [0, m, m, 2 * m])
    _same_radius(shell_reg.radiusSearch(sh.queries, r, sorted=True), want, f"m = {m}")
    _same_sets(shell_reg.radiusSearch(sh.queries, r, sorted=False), want)


@pytest.mark.parametrize("copies", [1, 2])
def test_radius_sort_with_ties_across_tiles(gpu, copies):
    """12 x 12 x 12 sites: a radius that takes them all gives segments of 1 728 and 3 456 entries, two and four tiles, full of equal
    distances, so a rank is right only if the (d2, index) order holds across tiles.  And radii whose square IS a lattice distance: strict."""
    lat = knn_cases.lattice(shape=(12, 12, 12), copies=copies, seed=61)
    q = np.zeros((5, 4), np.float32)
    q[0, :3] = (5, 6, 5); q[1, :3] = (5.5, 5.5, 6.5); q[2, :3] = (0, 11, 0); q[3, :3] = (5.5, 6, 5); q[4, :3] = (6, 4.5, 5.5)      # site, cell centre, corner, edge midpoint, face centre
    reg = LoamRegister()
    reg.setTarget(lat.target)
    want = knn_ref.radius_search(lat.target, q, 25.0)
    np.testing.assert_array_equal(np.diff(want[0].astype(np.int64)), [1728 * copies] * 5)
    assert (np.diff(want[2]) == 0).sum() > 5 * 1500 * copies
    _same_radius(reg.radiusSearch(q, 25.0), want, "the whole lattice")
    _same_sets(reg.radiusSearch(q, 25.0, sorted=False), want)
    _, d_all = knn_ref.knn(lat.target, q, 200)
    for r in (1.0, 1.5, 2.0):
        assert (d_all == r * r).sum() >= 6 * copies      # points at exactly r: out
        want = knn_ref.radius_search(lat.target, q, r)
        assert (want[2] < r * r).all()
        _same_radius(reg.radiusSearch(q, r), want, f"r = {r}")


@pytest.mark.parametrize("n_q", knn_cases.MIXED_SIZES)
def test_radius_counts_across_the_scan_chunks(cloud_reg, cloud, n_q):
    """queries with and without hits on both sides of every 1024-count chunk of radius_scan_kernel"""
    mq = knn_cases.mixed_queries(n_q, cloud["target"], seed=42)
    want = knn_ref.radius_search(cloud["target"], mq.queries, mq.values)
    got = cloud_reg.radiusSearch(mq.queries, mq.values)
    assert int(got[0][n_q]) == len(got[1]) == len(want[1])
    _same_radius(got, want, f"n_q = {n_q}")


# ---- 9: the host's query chunks -----------------------------------------------------------------------------------------------------------
def test_the_query_chunk_seam(gpu):
    """2^20 + 3 queries: pcr_knn's second chunk holds the last three, and the rows on both sides of the seam are copies of target points"""
    n_q = (1 << 20) + 3
    target = knn_cases.random_cloud(64, seed=51)
    q = knn_cases.random_queries(n_q, target, seed=52, spread=2.0)
    q[(1 << 20) - 1] = target[3]; q[1 << 20] = target[60]; q[(1 << 20) + 1] = target[17]
    q[:, 3] = 0
    reg = LoamRegister()
    reg.setTarget(target)
    want_i, want_d = knn_ref.knn(target, q, 2, chunk=4096)
    np.testing.assert_array_equal(want_i[(1 << 20) - 1:(1 << 20) + 2, 0], [3, 60, 17])
    _same_knn(reg.knn(q, 2), want_i, want_d, "2^20 + 3 queries")
