"""pcr_sc_rank_stored (stored ScanContexts ranked against each other on the device, csrc/scancontext.hip: sc_rank_stored_kernel +
sc_rank_merge_kernel) and the mirrors' rankStored / findLoops against the reference ranking of tests/sc_rank_ref.py over the CPU
oracle: indices and shifts equal, distances equal to the bit, and every reported pair equal to the library's own pcr_sc_distance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from simpleslam_amd import ScanContext
from tests import sc_rank_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = R.DBL_MAX
TILE_Q, TILE_C = 8, 128        # kTileQ, kTileC of csrc/scancontext.hip: queries kept in LDS per block, candidates streamed past them per block
EXCL = 3
N_ALL = 160


@pytest.fixture(autouse=True)
def _need_gpu(gpu):
    return gpu


def _clouds():
    """160 places of a few hundred points; among the first 150: two pairs of identical clouds, one cloud turned by exactly 3 sectors,
    three empty contexts (no point; every point beyond 80 m; only non-finite points -- that one at the candidate-tile edge) and a
    context with a single occupied column.  -> (clouds for the device, clouds for the oracle)"""
    cl = [R.make_scan(1000 + i, n=300, reach=85.0) for i in range(N_ALL)]
    cl[20] = cl[5].copy()
    cl[140] = cl[126].copy()
    cl[30] = R.rotate_sectors(cl[10], 3)
    cl[40] = np.zeros((0, 8), np.float32)
    far = R.make_scan(7, n=50)
    far[:, :2] *= (100.0 / np.linalg.norm(far[:, :2], axis=1))[:, None].astype(np.float32)
    cl[41] = far
    bad = R.make_scan(8, n=60)
    bad[0::3, 0], bad[1::3, 1], bad[2::3, 2] = np.nan, np.inf, np.nan
    cl[TILE_C - 1] = bad
    col = np.zeros((40, 8), np.float32)
    r = np.linspace(1.0, 75.0, 40)
    col[:, 0], col[:, 1], col[:, 2], col[:, 3] = r * np.cos(0.05), r * np.sin(0.05), np.linspace(-1.0, 4.0, 40), 1
    cl[50] = col
    for_oracle = list(cl)
    for_oracle[TILE_C - 1] = np.zeros((0, 8), np.float32)      # int(ceil(NaN)) is undefined in the reference; the device skips such points
    return cl, for_oracle


@pytest.fixture(scope="module")
def world():
    """the clouds, the oracle over all of them and its (dist, shift) of every ordered pair: computed once, never changed"""
    cl, for_oracle = _clouds()
    orc = oracle.ScanContextOracle(num_exclude_recent=EXCL)
    for c in for_oracle:
        orc.add(c)
    assert np.count_nonzero(orc.descriptor(50).any(0)) == 1            # the single occupied column
    for e in (40, 41, TILE_C - 1):
        assert not orc.descriptor(e).any()
    return {"clouds": cl, "orc": orc, "table": R.pair_table(orc), "dbs": {}}


def _db(world, n, **prm):
    """a database of the first n clouds (kept for the other tests of this module)"""
    key = (n, tuple(sorted(prm.items())))
    if key not in world["dbs"]:
        sc = ScanContext(**(prm or dict(num_exclude_recent=EXCL)))
        for c in world["clouds"][:n]:
            sc.addContext(c)
        world["dbs"][key] = sc
    return world["dbs"][key]


def _compare(sc, orc, table, first, count, k):
    idx, dist, shift = sc.rankStored(first, count, k)
    ri, rd, rs = R.rank(orc, first, count, k, table)
    assert idx.shape == (count, k) and idx.dtype == np.int64 and dist.dtype == np.float64 and shift.dtype == np.int32
    bad = np.argwhere((idx != ri) | (shift != rs) | (dist.view(np.uint64) != rd.view(np.uint64)))
    assert bad.size == 0, (first, count, k, [(int(r) + first, int(c), int(idx[r, c]), int(ri[r, c]), dist[r, c], rd[r, c], int(shift[r, c]), int(rs[r, c]))
                                            for r, c in bad[:5]])
    for row, col in np.argwhere(idx >= 0):                             # the library's own host path, pair by pair
        assert (dist[row, col], shift[row, col]) == sc.distance(first + row, int(idx[row, col])), (first + row, idx[row, col])
    return idx, dist, shift


@pytest.mark.parametrize("k", [1, 8])
def test_whole_triangle_equals_the_reference_to_the_bit(world, k):
    n = 150
    sc = _db(world, n)
    idx, dist, shift = _compare(sc, world["orc"], world["table"], 0, n, k)
    assert (idx[:EXCL + 1] == -1).all()
    assert idx[30, 0] == 10 and shift[30, 0] == 3                      # the cloud turned by 3 sectors finds its original, at shift 3
    assert idx[20, 0] == 5 and idx[140, 0] == 126                      # the identical clouds find each other ...
    d5, d20 = sc.distance(60, 5), sc.distance(60, 20)                  # ... and tie for everyone else: the reference lists 5 before 20
    assert d5 == d20
    if k == 8:
        for q in range(24, n):
            at = idx[q].tolist()
            assert (20 not in at) or at.index(20) == at.index(5) + 1, (q, at)
    assert sc.distance(60, 40) == (DBL_MAX, 0) and sc.distance(60, 41) == (DBL_MAX, 0) and sc.distance(140, TILE_C - 1) == (DBL_MAX, 0)
    assert idx[40].tolist() == list(range(k)) and (dist[40] == DBL_MAX).all()      # an empty query: every candidate at DBL_MAX, by index


def test_tile_edges(world):
    """Database sizes and windows one below, at and one above the query tile (8) and the candidate tile (128; with 3 recent contexts
    excluded, the last query's candidates end at n - 4), windows that start and end inside a tile, and the last id alone."""
    orc, table = world["orc"], world["table"]
    for n in (TILE_Q - 1, TILE_Q, TILE_Q + 1, TILE_C - 1, TILE_C, TILE_C + 1, TILE_C + EXCL, TILE_C + EXCL + 1, TILE_C + EXCL + 2):
        sc = _db(world, n)
        _compare(sc, orc, table, 0, n, 2)
        _compare(sc, orc, table, n - 1, 1, 8)                          # count = 1 at the last id
    sc = _db(world, N_ALL)
    for first, count in ((0, TILE_Q - 1), (0, TILE_Q), (0, TILE_Q + 1), (5, TILE_Q), (TILE_C - 1, 1), (TILE_C - 1, TILE_Q + 1), (TILE_C, TILE_Q),
                         (TILE_C + EXCL - 2, 5), (TILE_C + EXCL - 1, 1), (TILE_C + EXCL, 1), (TILE_C + EXCL + 1, 1), (3, 150), (N_ALL - 1, 1),
                         (N_ALL - TILE_Q - 1, TILE_Q + 1)):
        _compare(sc, orc, table, first, count, 3)
    _compare(sc, orc, table, 0, N_ALL, 8)


def test_default_parameters(world):
    n = 64
    sc = _db(world, n, num_exclude_recent=40)
    orc40 = oracle.ScanContextOracle()                                 # num_exclude_recent = 40
    orc40.polar, orc40.ring, orc40.sector = world["orc"].polar[:n], world["orc"].ring[:n], world["orc"].sector[:n]
    idx, dist, shift = _compare(sc, orc40, world["table"], 0, n, 8)
    assert (idx[:41] == -1).all() and (dist[:41] == DBL_MAX).all() and (shift[:41] == 0).all()
    for q in range(41, n):
        have = min(8, q - 40)                                          # 1 .. 23 candidates
        assert (idx[q, :have] >= 0).all() and (idx[q, :have] < q - 40).all()
        assert (idx[q, have:] == -1).all() and (dist[q, have:] == DBL_MAX).all() and (shift[q, have:] == 0).all()
    loops = sc.findLoops()
    assert loops == R.find_loops(orc40, 0, n, world["table"])
    assert loops[:41] == [(q, -1, np.float32(0), None) for q in range(41)]


def test_against_query_on_a_trajectory_that_revisits_its_start():
    """70 places, then the first 30 revisited with a yaw of 11 sectors and noise, default parameters.  The exhaustive ranking is never
    worse than query's 10 ring-key candidates; where both pick the same context they agree to the bit; and ranking between two query
    calls leaves the second as it would have been."""
    rng = np.random.default_rng(0)
    places = [R.make_scan(100 + i, n=600, reach=75.0) for i in range(70)]
    a, b = ScanContext(), ScanContext()
    got = []
    for step, pl in enumerate(list(range(70)) + list(range(30))):
        c = places[pl]
        if step >= 70:
            c = R.rotate_sectors(c, 11)
            c[:, :3] += rng.normal(0, 0.01, (c.shape[0], 3)).astype(np.float32)
        a.addContext(c)
        b.addContext(c)
        if step % 3 == 0:
            b.rankStored(0, step + 1, 2)                               # between b's query calls: must not move its candidate snapshot
        qa, qb = a.query(step), b.query(step)
        assert qa == qb, (step, qa, qb)
        got.append(qa)
    loops = a.findLoops()
    assert loops == b.findLoops(0, 100) and len(loops) == 100
    idx, dist, shift = a.rankStored(0, 100, 1)
    found = same = 0
    for step, (m, yaw, d) in enumerate(got):
        lid, lm, lyaw, ld = loops[step]
        assert lid == step
        if d is not None:
            assert ld is not None and ld <= d, (step, ld, d)         # query's candidates are among the ranking's
        if m < 0:
            continue
        found += 1
        assert lm >= 0
        if lm == m:
            same += 1
            assert ld == d and lyaw == yaw and lyaw.dtype == yaw.dtype == np.float32
            assert shift[step, 0] == a.distance(step, m)[1] and idx[step, 0] == m
        if step >= 70:
            assert lm == step - 70 and abs(float(lyaw) - np.deg2rad(66.0)) < 1e-6
    assert found >= 20 and same >= 20


def test_repeatable_and_independent_of_the_window(world):
    n = 150
    sc = _db(world, n)
    one = sc.rankStored(0, n, 8)
    two = sc.rankStored(0, n, 8)
    for x, y in zip(one, two):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
    parts = [sc.rankStored(0, 47, 8), sc.rankStored(47, 60, 8), sc.rankStored(107, 43, 8)]
    for j, x in enumerate(one):
        cat = np.concatenate([p[j] for p in parts])
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, cat.view(np.uint64) if cat.dtype == np.float64 else cat)


def test_refusals_write_nothing(world):
    n = 64
    sc = _db(world, n, num_exclude_recent=40)
    lib, h = sc._lib, sc._s
    idx, dist, shift = np.full((n + 1, 8), 77, np.int64), np.full((n + 1, 8), 7.5), np.full((n + 1, 8), 77, np.int32)
    pi, pd, ps = idx.ctypes.data_as(C.POINTER(C.c_int64)), dist.ctypes.data_as(C.POINTER(C.c_double)), shift.ctypes.data_as(C.POINTER(C.c_int32))

    def refused(first, count, k, a, b, c, word):
        assert lib.pcr_sc_rank_stored(h, first, count, k, a, b, c) != 0
        assert word in lib.pcr_sc_last_error(h).decode(), lib.pcr_sc_last_error(h)
        assert (idx == 77).all() and (dist == 7.5).all() and (shift == 77).all()

    refused(0, n, 0, pi, pd, ps, "k ")
    refused(0, n, 9, pi, pd, ps, "k ")
    refused(0, n + 1, 1, pi, pd, ps, "first + count")
    refused(n, 1, 1, pi, pd, ps, "first + count")
    refused(2**63, 2**63, 1, pi, pd, ps, "first + count")              # (a sum that wraps)
    refused(0, n, 1, None, pd, ps, "idx")
    refused(0, n, 1, pi, None, ps, "dist")
    refused(0, n, 1, pi, pd, None, "shift")
    assert lib.pcr_sc_rank_stored(h, 0, 0, 1, pi, pd, ps) == 0
    assert lib.pcr_sc_rank_stored(h, n, 0, 1, None, None, None) == 0
    assert (idx == 77).all() and (dist == 7.5).all() and (shift == 77).all()
    with pytest.raises(Exception):
        sc.rankStored(0, n, 9)
    with pytest.raises(Exception):
        sc.findLoops(60, 5)
    empty = ScanContext()
    assert lib.pcr_sc_rank_stored(empty._s, 0, 0, 1, pi, pd, ps) == 0
    assert empty.findLoops() == [] and empty.rankStored(0, 0, 3)[0].shape == (0, 3)
    assert lib.pcr_sc_rank_stored(empty._s, 0, 1, 1, pi, pd, ps) != 0
    assert lib.pcr_sc_rank_stored(h, 0, n, 8, pi, pd, ps) == 0          # ... and the handle still serves
    assert (idx[n] == 77).all() and (idx[:41] == -1).all()


def test_sc_loops_check_program():
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "sc_loops_check")
    assert os.path.exists(exe), "sc_loops_check not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "sc_loops_check ok"
