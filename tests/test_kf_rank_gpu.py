"""pcr_map_rank_near on the device against pcr_kf_rank_near_host, bit for bit, on stores of one-point key frames where only the poses matter:
the host test's cases, sizes at the edges of the kernel's tiles, a walk that revisits itself, windows, new poses and a view."""
import ctypes as C

import numpy as np
import pytest

from kf_rank_cases import REFUSALS, random_walk, small_cases

pytestmark = pytest.mark.gpu
CASES = small_cases()
TILE_Q, TILE_C = 16, 256      # kf_rank.hip: kTileQ queries per block, kTileC candidates per staged tile
ONE_POINT = np.array([[0.5, 0.25, 0.125, 1.0]], np.float32)


def poses_at(xyz):
    P = np.tile(np.eye(4), (len(xyz), 1, 1))
    P[:, :3, 3] = xyz
    return P


@pytest.fixture(scope="module")
def store(gpu):
    """One store for the whole module, refilled per test: fill(xyz) -> the SubMap with one key frame per position."""
    from simpleslam_amd import SubMap
    sm = SubMap()

    def fill(xyz):
        sm.clear()
        for P in poses_at(np.asarray(xyz, dtype=np.float64).reshape(-1, 3)):
            sm.addKeyFrame(ONE_POINT, P)
        return sm
    return fill


def assert_equals_host(sm, xyz, first, count, excl, radius, k):
    from simpleslam_amd import kf_rank_near_host
    idx, d2 = sm.rankNear(first, count, radius, k=k, num_exclude_recent=excl)
    ref_idx, ref_d2 = kf_rank_near_host(xyz, first, count, radius, k=k, num_exclude_recent=excl)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(d2.view(np.uint64), ref_d2.view(np.uint64))
    return idx, d2


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_host_tests_cases(store, case):
    _name, xyz, excl, radius = case
    sm = store(xyz)
    for k in (1, 8):
        assert_equals_host(sm, xyz, 0, xyz.shape[0], excl, radius, k)


@pytest.mark.parametrize("n", [TILE_Q - 1, TILE_Q, TILE_Q + 1, TILE_C - 1, TILE_C, TILE_C + 1, 2 * TILE_C + 1])
def test_sizes_at_the_tile_edges(store, n):
    xyz = random_walk(n, 100 + n, step=0.2)      # (a small course: most key frames lie within the radius of many others)
    sm = store(xyz)
    for k, excl in ((1, 0), (8, 0), (3, 5)):
        idx, _ = assert_equals_host(sm, xyz, 0, n, excl, 4.0, k)
        assert (idx[-1] >= 0).all()


@pytest.fixture(scope="module")
def walk(store):
    xyz = random_walk(3000, 7)
    return store(xyz), xyz


@pytest.mark.parametrize("k", [1, 8])
def test_a_walk_of_3000_key_frames_and_its_windows(walk, k):
    sm, xyz = walk
    idx, d2 = assert_equals_host(sm, xyz, 0, 3000, 40, 2.5, k)
    assert (idx[:, 0] >= 0).sum() > 2000 and (idx[:, -1] < 0).any()
    # a row depends on its query alone: the same bits whatever the window, tile-aligned or not
    for first, count in ((0, 1), (2999, 1), (1234, 1), (7, 300), (2000, 1000), (TILE_Q * 50, TILE_Q * 3), (TILE_Q * 50 + 3, TILE_Q * 3 + 5)):
        w_idx, w_d2 = sm.rankNear(first, count, 2.5, k=k, num_exclude_recent=40)
        np.testing.assert_array_equal(w_idx, idx[first:first + count])
        np.testing.assert_array_equal(w_d2.view(np.uint64), d2[first:first + count].view(np.uint64))


def test_new_poses_and_a_view(walk):
    sm, xyz = walk
    view = sm.view()
    before = sm.rankNear(0, 3000, 2.5, k=8, num_exclude_recent=40)
    for a, b in zip(view.rankNear(0, 3000, 2.5, k=8, num_exclude_recent=40), before):
        np.testing.assert_array_equal(a, b)
    moved = xyz.copy()
    moved[1000:2000] += [0.7, -0.4, 0.1]
    sm.setPoses(1000, poses_at(moved[1000:2000]))
    try:
        after = assert_equals_host(sm, moved, 0, 3000, 40, 2.5, 8)
        assert not np.array_equal(after[0], before[0])
        for a, b in zip(view.rankNear(500, 2000, 2.5, k=8, num_exclude_recent=40), after):      # (the view reads the parent's poses)
            np.testing.assert_array_equal(a, b[500:2500])
    finally:
        sm.setPoses(1000, poses_at(xyz[1000:2000]))


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing_and_leave_a_message(store, name, change):
    from simpleslam_amd import load_library
    lib = load_library()
    sm = store(np.arange(18, dtype=np.float64).reshape(6, 3))
    a = dict(first=0, count=6, excl=0, radius=100.0, k=2, null=None)
    a.update(change)
    idx, d2 = np.full((8, 8), -77, np.int64), np.full((8, 8), -77.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rc = lib.pcr_map_rank_near(sm._m, a["first"], a["count"], a["excl"], a["radius"], a["k"],
                               None if a["null"] == "idx" else idx.ctypes.data_as(ip), None if a["null"] == "d2" else d2.ctypes.data_as(dp))
    assert rc != 0 and lib.pcr_map_last_error(sm._m).decode().startswith("pcr_map_rank_near: ")
    assert np.all(idx == -77) and np.all(d2 == -77.0)
    assert lib.pcr_map_rank_near(sm._m, 6, 0, 0, 1.0, 1, None, None) == 0      # count == 0
