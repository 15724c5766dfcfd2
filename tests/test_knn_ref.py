"""tests/knn_ref.py, the numpy restatement pcr_knn and pcr_radius_search are checked against, held to the reference's own nanoflann
(the recorded answers under tests/golden); and the two entry points' presence in the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import knn_ref

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def more():
    return np.load(os.path.join(G, "ref_nanoflann_more.npz"))


def test_knn_reproduces_the_reference_k5(more):
    idx, d2 = knn_ref.knn(more["knn_points"], more["knn_queries"], 5)
    np.testing.assert_array_equal(idx, more["knn_idx"])
    assert d2.tobytes() == more["knn_d2"].tobytes()      # bit for bit


def test_knn_reproduces_the_first_golden_cloud():
    """knn_nanoflann.npz has queries placed next to duplicated points: the distances are the reference's bit for bit, and where a row's
    distances are all different so are the indices (nanoflann orders equal distances by its tree walk, knn_ref by index)."""
    z = np.load(os.path.join(G, "knn_nanoflann.npz"))
    idx, d2 = knn_ref.knn(z["points"], z["queries"], 5)
    assert d2.tobytes() == z["d2"].tobytes()
    idx6, d6 = knn_ref.knn(z["points"], z["queries"], 6)
    untied = (np.diff(d6, axis=1) != 0).all(axis=1)
    assert untied.sum() >= 384
    np.testing.assert_array_equal(idx[untied], z["idx"][untied])
    # tied rows: the same points up to the order of coincident ones
    pts = z["points"][:, :3]
    np.testing.assert_array_equal(pts[idx], pts[z["idx"]])


def test_radius_reproduces_the_reference_lists(more):
    """ref_nanoflann_live.npz: radiusSearch(r = 0.75) of the first 32 golden queries, in the tree's order"""
    live = np.load(os.path.join(G, "ref_nanoflann_live.npz"))
    q = more["knn_queries"][:32]
    off, idx, d2 = knn_ref.radius_search(more["knn_points"], q, 0.75, sorted_=True)
    np.testing.assert_array_equal(np.diff(off.astype(np.int64)), live["radius_counts"])
    ends = np.cumsum(live["radius_counts"])
    for j, (e, n) in enumerate(zip(ends, live["radius_counts"])):
        ri, rd = live["radius_idx"][e - n:e], live["radius_d2"][e - n:e]
        o = np.lexsort((ri, rd))
        a, b = int(off[j]), int(off[j + 1])
        np.testing.assert_array_equal(idx[a:b], ri[o])
        assert d2[a:b].tobytes() == rd[o].tobytes()
    off_u, idx_u, _ = knn_ref.radius_search(more["knn_points"], q, 0.75, sorted_=False)
    np.testing.assert_array_equal(off_u, off)
    for j in range(32):
        a, b = int(off[j]), int(off[j + 1])
        np.testing.assert_array_equal(np.sort(idx_u[a:b]), np.sort(idx[a:b]))


def test_semantics_of_the_edges():
    pts = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [np.nan, 0, 0, 0], [2, 0, 0, 0], [5, 0, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [np.inf, 0, 0]], np.float32)
    idx, d2 = knn_ref.knn(pts, q, 5)
    np.testing.assert_array_equal(idx, [[0, 1, 3, 4, -1], [-1] * 5])      # the NaN point is skipped and renumbers nothing; ties by row
    np.testing.assert_array_equal(d2[0], [0, 4, 4, 25, np.inf])
    off, ridx, _ = knn_ref.radius_search(pts, q, 2.0)
    np.testing.assert_array_equal(off, [0, 1, 1])                          # distance exactly r is outside
    off, ridx, _ = knn_ref.radius_search(pts, q, np.nextafter(2.0, np.inf))
    np.testing.assert_array_equal(off, [0, 3, 3])
    np.testing.assert_array_equal(ridx, [0, 1, 3])


def test_library_exports_the_queries():
    """the built library has both entry points, and a NULL handle is refused with 1 (nothing touches a device)"""
    import simpleslam_amd
    lib = simpleslam_amd.load_library()
    assert hasattr(lib, "pcr_knn") and hasattr(lib, "pcr_radius_search")
    from simpleslam_amd.pcr import ABI_SYMBOLS
    assert "pcr_knn" in ABI_SYMBOLS and "pcr_radius_search" in ABI_SYMBOLS
    idx, d2 = (C.c_int64 * 1)(), (C.c_double * 1)()
    q = (C.c_float * 4)()
    assert lib.pcr_knn(None, q, 1, 16, 0, 1, idx, d2) == 1
    off, tot = (C.c_uint64 * 2)(), C.c_size_t(0)
    assert lib.pcr_radius_search(None, q, 1, 16, 0, 1.0, 1, 1, off, idx, d2, C.byref(tot)) == 1
