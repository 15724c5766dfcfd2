"""pcr_kf_rank_near_host, the definition of the key-frame ranking by distance, against a numpy brute force with the same rounding order:
exact equality of idx and d2 (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from kf_rank_cases import DBL_MAX, REFUSALS, brute, random_walk, small_cases

CASES = small_cases()


@pytest.fixture(scope="module")
def lib():
    import simpleslam_amd
    return simpleslam_amd.load_library()


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_small_cases_equal_the_brute_force(case, k):
    from simpleslam_amd import kf_rank_near_host
    _name, xyz, excl, radius = case
    n = xyz.shape[0]
    idx, d2 = kf_rank_near_host(xyz, 0, n, radius, k=k, num_exclude_recent=excl)
    ref_idx, ref_d2 = brute(xyz, 0, n, excl, radius, k)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(d2, ref_d2)


def test_the_cases_hold_what_they_are_named_for():
    """The brute force itself, at the rows the cases were built for: were it to drop a tie or a boundary, the comparison above would prove less."""
    by_name = {c[0]: c for c in CASES}
    _n, xyz, excl, radius = by_name["d2 equals radius^2 is in, the next double above is out"]
    idx, d2 = brute(xyz, 4, 1, excl, radius, 8)
    assert idx[0].tolist() == [0, 2, -1, -1, -1, -1, -1, -1] and d2[0, 0] == 25.0 and d2[0, 2] == DBL_MAX
    _n, xyz, excl, radius = by_name["mirrored about the query"]
    idx, d2 = brute(xyz, 8, 1, excl, radius, 8)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and np.all(d2[0] == 9.0)
    _n, xyz, excl, radius = by_name["radius 0 with a duplicate"]
    assert brute(xyz, 2, 1, excl, radius, 1)[0].tolist() == [[0]]
    _n, xyz, excl, radius = by_name["n is the exclusion plus one"]
    assert brute(xyz, 0, 4, excl, radius, 1)[0][:, 0].tolist() == [-1, -1, -1, -1]
    _n, xyz, excl, radius = by_name["n is the exclusion plus two: the first query with one candidate"]
    assert brute(xyz, 0, 5, excl, radius, 1)[0][:, 0].tolist() == [-1, -1, -1, -1, 0]
    _n, xyz, excl, radius = by_name["a NaN and an Inf as candidates"]
    assert brute(xyz, 5, 1, excl, radius, 8)[0][0].tolist() == [0, 3, -1, -1, -1, -1, -1, -1]
    _n, xyz, excl, radius = by_name["an Inf under a radius whose square overflows"]
    assert brute(xyz, 3, 1, excl, radius, 8)[0][0].tolist() == [2, 0, -1, -1, -1, -1, -1, -1]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_a_walk_that_revisits_itself_and_its_windows(k):
    from simpleslam_amd import kf_rank_near_host
    xyz = random_walk(700, 11)
    idx, d2 = kf_rank_near_host(xyz, 0, 700, 2.5, k=k, num_exclude_recent=40)
    ref_idx, ref_d2 = brute(xyz, 0, 700, 40, 2.5, k)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(d2, ref_d2)
    assert (idx[:, 0] >= 0).sum() > 100 and (idx[:, -1] < 0).any()      # (loops are found, and some rows have a tail)
    for first, count in ((0, 1), (699, 1), (333, 17), (200, 500)):
        w_idx, w_d2 = kf_rank_near_host(xyz, first, count, 2.5, k=k, num_exclude_recent=40)
        np.testing.assert_array_equal(w_idx, idx[first:first + count])
        np.testing.assert_array_equal(w_d2, d2[first:first + count])


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(lib, name, change):
    xyz = np.ascontiguousarray(np.arange(18, dtype=np.float64).reshape(6, 3))
    a = dict(first=0, count=6, excl=0, radius=100.0, k=2, null=None)
    a.update(change)
    idx, d2 = np.full((8, 8), -77, np.int64), np.full((8, 8), -77.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rc = lib.pcr_kf_rank_near_host(xyz.ctypes.data_as(dp), 6, a["first"], a["count"], a["excl"], a["radius"], a["k"],
                                   None if a["null"] == "idx" else idx.ctypes.data_as(ip), None if a["null"] == "d2" else d2.ctypes.data_as(dp))
    assert rc != 0
    assert np.all(idx == -77) and np.all(d2 == -77.0)


def test_count_zero_returns_zero_and_writes_nothing(lib):
    xyz = np.zeros((4, 3))
    dp = C.POINTER(C.c_double)
    assert lib.pcr_kf_rank_near_host(xyz.ctypes.data_as(dp), 4, 4, 0, 0, 1.0, 1, None, None) == 0
    assert lib.pcr_kf_rank_near_host(None, 0, 0, 0, 0, 1.0, 8, None, None) == 0
