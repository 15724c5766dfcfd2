"""tests/voxel_sparse_ref.py -- the restatement of pcp::VoxelDownSampleV3 and pcp::VoxelDownSampleV2 the device tests compare with -- checked
by itself: hand-worked tables for both kinds, V3 against the restatement of pcl::VoxelGrid (tests/voxel_ref.py) wherever PCL's too-fine test
does not refuse, V2's double-width voxels about zero, its cap and its strict min_voxel_pts, and the 64 / 65-bit decision.  No GPU."""
import numpy as np
import pytest

import voxel_ref as V
import voxel_sparse_ref as S


def _xyz(rows, stride=4):
    a = np.zeros((len(rows), stride), np.float32)
    a[:, :len(rows[0])] = rows
    return a


def test_v3_hand_worked_table():
    # leaf 0.5 (inv = 2 exactly): floor(2 p) per axis.  Rows:       lattice          relative to min (-3, 0, 0)
    pts = _xyz([[0.10, 0.10, 0.10, 1.0],       #  0: ( 0, 0, 0)        (3, 0, 0)
                [0.40, 0.20, 0.30, 3.0],       #  1: ( 0, 0, 0)        (3, 0, 0)
                [-1.25, 0.00, 0.00, 5.0],      #  2: (-3, 0, 0)        (0, 0, 0)
                [0.60, 0.70, 0.00, 7.0],       #  3: ( 1, 1, 0)        (4, 1, 0)
                [np.nan, 0.0, 0.0, 9.0],       #  4: dropped
                [0.10, 0.10, 1.20, 11.0],      #  5: ( 0, 0, 2)        (3, 0, 2)
                [0.0, np.inf, 0.0, 13.0]])     #  6: dropped
    r = S.sparse_ref(pts, 0.5, S.V3)
    assert r.kept.tolist() == [True, True, True, True, False, True, False]
    assert r.rel.tolist() == [[3, 0, 0], [3, 0, 0], [0, 0, 0], [4, 1, 0], [3, 0, 2]]
    assert r.extents == (5, 2, 3) and r.bits == (3, 1, 2)
    # key = x | y << 3 | z << 4
    assert r.keys.tolist() == [3, 3, 0, 4 | 8, 3 | 32]
    k, rows = r.sorted_pairs()
    assert k.tolist() == [0, 3, 3, 12, 35] and rows.tolist() == [2, 0, 1, 3, 5]
    # ascending (z, y, x): (0,0,0), (3,0,0), (4,1,0), (3,0,2)
    assert r.members == [[2], [0, 1], [3], [5]]
    want = _xyz([[-1.25, 0.0, 0.0, 5.0], [0.25, 0.15, 0.2, 2.0], [0.6, 0.7, 0.0, 7.0], [0.1, 0.1, 1.2, 11.0]])
    assert S.ulp_distance(r.out, want).max() <= 1
    # the 32-byte layout: data[3] = 1, the intensity is float 4, everything else zero
    p8 = np.zeros((len(pts), 8), np.float32)
    p8[:, :3] = pts[:, :3]; p8[:, 3] = 1.0; p8[:, 4] = pts[:, 3]; p8[:, 5:] = 42.0
    r8 = S.sparse_ref(p8, 0.5, S.V3)
    np.testing.assert_array_equal(r8.out[:, 3], 1.0)
    np.testing.assert_array_equal(r8.out[:, 5:], 0.0)
    np.testing.assert_array_equal(r8.out[:, 4], r.out[:, 3])
    np.testing.assert_array_equal(r8.out[:, :3], r.out[:, :3])


def test_v2_hand_worked_table_and_double_width_voxels_about_zero():
    # leaf 0.5: (int)(p / 0.5) truncates toward zero, so -0.49 .. 0.49 is ONE voxel on an axis, two leaves wide
    pts = _xyz([[0.40, 0.0, 0.0, 1.0],         # 0: ( 0, 0, 0)
                [-0.40, 0.0, 0.0, 2.0],        # 1: ( 0, 0, 0)   (floor would say -1)
                [-0.60, 0.0, 0.0, 3.0],        # 2: (-1, 0, 0)
                [0.60, 0.0, 0.0, 4.0],         # 3: ( 1, 0, 0)
                [0.20, -0.30, 0.45, 5.0],      # 4: ( 0, 0, 0)
                [0.20, -0.30, -0.55, 6.0],     # 5: ( 0, 0, -1)
                [np.nan, 0.0, 0.0, 7.0]])      # 6: dropped
    r = S.sparse_ref(pts, 0.5, S.V2)
    assert r.rel.tolist() == [[1, 0, 1], [1, 0, 1], [0, 0, 1], [2, 0, 1], [1, 0, 1], [1, 0, 0]]
    assert r.extents == (3, 1, 2) and r.bits == (2, 0, 1)
    assert r.keys.tolist() == [5, 5, 4, 6, 5, 1]
    assert r.members == [[5], [2], [0, 1, 4], [3]]
    assert r.out_rows.tolist() == [5, 2, 0, 3]
    f = np.float32
    m = ((f(0) + f(0.40)) + f(-0.40) + f(0.20)) / f(3)
    np.testing.assert_array_equal(r.out[2], np.array([m, ((f(0) + f(0)) + f(0) + f(-0.30)) / f(3), ((f(0) + f(0)) + f(0) + f(0.45)) / f(3), 1.0], f))
    np.testing.assert_array_equal(r.out[0], pts[5])      # a voxel of one row: (0 + x) / 1
    # V3 on the same cloud separates what V2 joins about zero
    assert len(S.sparse_ref(pts, 0.5, S.V3).out) == 6


def test_v2_cap_and_strict_min_voxel_pts():
    rng = np.random.default_rng(3)
    a = np.zeros((30, 4), np.float32)
    a[:, :3] = 1.0 + 0.4 * rng.random((30, 3), dtype=np.float32)       # one voxel at leaf 0.5: (2, 2, 2) .. all within [1.0, 1.5)
    a[:, 3] = np.arange(30)
    a[25, :3] = [1.49, 1.49, 1.49]
    for cap in (1, 5, 29, 30, 31):
        r = S.sparse_ref(a, 0.5, S.V2, max_voxel_pts=cap)
        assert r.members == [list(range(min(cap, 30)))]
        s = np.zeros(3, np.float32)
        for i in range(min(cap, 30)):
            s = s + a[i, :3]
        np.testing.assert_array_equal(r.out[0, :3], s / np.float32(min(cap, 30)))
        assert r.out[0, 3] == 0.0                                      # the first row's record
    # strict: a voxel that kept c rows is emitted for min_voxel_pts < c only; the cap counts first
    assert len(S.sparse_ref(a, 0.5, S.V2, 20, 19).out) == 1
    assert len(S.sparse_ref(a, 0.5, S.V2, 20, 20).out) == 0
    assert len(S.sparse_ref(a, 0.5, S.V2, 40, 29).out) == 1
    assert len(S.sparse_ref(a, 0.5, S.V2, 40, 30).out) == 0
    # a permutation keeps other rows
    p = a[::-1].copy()
    assert S.sparse_ref(p, 0.5, S.V2, 5).out[0, 3] == 29.0
    assert not np.array_equal(S.sparse_ref(p, 0.5, S.V2, 5).out[0, :3], S.sparse_ref(a, 0.5, S.V2, 5).out[0, :3])


def _against_pcl(pts, leaf):
    ref, r = V.voxel_ref(pts, leaf), S.sparse_ref(pts, leaf, S.V3)
    assert not ref.unfiltered
    assert len(r.out) == len(ref)
    for i in range(len(ref)):
        assert r.members[i] == ref.members(i).tolist()                  # the same voxels in the same order
    assert S.ulp_distance(r.out, ref.mean64).max() <= 1
    # the key orders the rows as PCL's index does
    k, rows = r.sorted_pairs()
    np.testing.assert_array_equal(rows, np.concatenate([ref.members(i) for i in range(len(ref))]))


@pytest.mark.parametrize("leaf,sign", [(0.05, 1.0), (0.1, -1.0), (0.3, 1.0), (0.25, -1.0)])
def test_v3_is_pcls_lattice_on_face_clouds(leaf, sign):
    pts, _ = V.face_cloud(leaf, sign, n=3000, seed=int(leaf * 100), only_disagreeing=leaf != 0.25)      # (an exact leaf: float and double agree on every face)
    _against_pcl(pts, leaf)


@pytest.mark.parametrize("leaf,log2_ratio,sign", [(0.05, 23.1, 1.0), (0.1, 24.0, -1.0), (0.3, 24.9, 1.0)])
def test_v3_is_pcls_lattice_far_from_the_origin(leaf, log2_ratio, sign):
    _against_pcl(V.far_cloud(leaf, log2_ratio, sign, n=3000, seed=7), leaf)


@pytest.mark.parametrize("name", ["duplicates", "lattice_0.1", "nan_axis0", "-inf_axis2"])
def test_v3_is_pcls_lattice_on_awkward_content(name):
    pts, leaf = V.awkward_clouds()[name]
    _against_pcl(pts, leaf)


def _corners(ex, leaf=1.0):
    """two rows at opposite corners of a box of ex = (ex, ey, ez) voxels at an exact leaf"""
    return _xyz([[0.0, 0.0, 0.0], [(ex[0] - 1) * leaf, (ex[1] - 1) * leaf, (ex[2] - 1) * leaf]])


def test_the_64_and_65_bit_decision():
    for kind in (S.V3, S.V2):
        r = S.sparse_ref(_corners((2 ** 22, 2 ** 21, 2 ** 21)), 1.0, kind)
        assert r.bits == (22, 21, 21) and int(r.keys[1]) == 2 ** 64 - 1 and int(r.keys[0]) == 0
        with pytest.raises(S.SparseRefused) as e:
            S.sparse_ref(_corners((2 ** 22, 2 ** 22, 2 ** 21)), 1.0, kind)
        assert e.value.why == "bits" and e.value.bits == 65 and e.value.extents == (2 ** 22, 2 ** 22, 2 ** 21)
        # an extent of 2^k + 1 takes k + 1 bits: one voxel more on an axis tips 64 into 65
        assert sum(S.sparse_ref(_corners((2 ** 22, 2 ** 21, 2 ** 21)), 1.0, kind).bits) == 64
        with pytest.raises(S.SparseRefused):
            S.sparse_ref(_corners((2 ** 22, 2 ** 21 + 1, 2 ** 21)), 1.0, kind)
        # extent 1 takes no bit
        assert S.sparse_ref(_corners((1, 1, 9)), 1.0, kind).bits == (0, 0, 4)


def test_int_range_refusal():
    for kind in (S.V3, S.V2):
        with pytest.raises(S.SparseRefused) as e:
            S.sparse_ref(_xyz([[0.0, 0.0, 0.0], [3.0e9, 0.0, 0.0]]), 1.0, kind)
        assert e.value.why == "range"
        S.sparse_ref(_xyz([[0.0, 0.0, 0.0], [-2.0 ** 31, 0.0, 0.0], [np.inf, 0, 0]]), 1.0, kind)      # INT_MIN itself is an int; inf is dropped
