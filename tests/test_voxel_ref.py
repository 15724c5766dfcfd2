"""CPU tests (no GPU): the voxel-filter oracle (oracle/voxel_oracle.c) against the plain numpy restatement of pcl::VoxelGrid in
tests/voxel_ref.py, exactly -- the same rows in the same order, the float32 sums bit for bit -- on clouds built to sit where float and
double arithmetic disagree about the voxel, and PCL's too-fine decision on thousands of boxes next to INT_MAX voxels."""
import collections

import numpy as np
import pytest

import oracle
import voxel_ref as V


def _widen(pts, stride):
    """the cloud's xyz (+ intensity) in a point of `stride` floats; any further floats are filled with noise the filter must ignore"""
    out = np.random.default_rng(stride).random((pts.shape[0], stride), dtype=np.float32) * 7
    out[:, :3] = pts[:, :3]
    ic = V.intensity_column(stride)
    if ic is not None:
        out[:, ic] = pts[:, 3]
    return out


def _adversarial():
    out = []
    for leaf in (0.05, 0.1, 0.3, 0.25, 0.5):
        for sign in (1.0, -1.0):
            pts, _ = V.face_cloud(leaf, sign, n=6000, seed=int(leaf * 100) + (sign > 0), only_disagreeing=leaf not in (0.25, 0.5))
            out.append((f"faces_{leaf}_{'+' if sign > 0 else '-'}", pts, leaf))
    for leaf, e, sign in ((0.05, 23.5, 1.0), (0.1, 24.0, -1.0), (0.3, 24.5, 1.0), (0.25, 23.2, -1.0)):
        out.append((f"far_{leaf}_2^{e}", V.far_cloud(leaf, e, sign, n=6000, seed=int(e * 10)), leaf))
    for name, (pts, leaf) in V.awkward_clouds(seed=3).items():
        if name == "voxel_sizes":
            pts = pts[np.abs(pts[:, 0] - 8.5) > 1.0]          # (the 100 000-point voxel: the GPU tests take it; the float32 sums here go point by point)
        out.append((name, pts, leaf))
    return out


ADVERSARIAL = _adversarial()


@pytest.mark.parametrize("stride", [3, 4, 5, 6, 8])
def test_oracle_equals_reference_exactly(stride):
    """12-, 16-, 20-, 24- and 32-byte points: every row of the oracle's output is the reference's, in the same order, bit for bit."""
    for name, pts, leaf in ADVERSARIAL:
        p = _widen(pts, stride)
        ref = V.voxel_ref(p, leaf)
        got, unfiltered = oracle.voxel_filter(p, leaf)
        assert unfiltered == ref.unfiltered, name
        assert got.shape == (len(ref), stride), name
        np.testing.assert_array_equal(got, ref.sum32, err_msg=name)
        # and the float32 sums are the float64 mean to float rounding: the two centroids of the reference describe the same voxels
        if len(ref):
            d = V.ulp_distance(ref.sum32[:, :3], ref.mean64[:, :3])
            assert np.all((d <= 64) | (np.abs(ref.sum32[:, :3] - ref.mean64[:, :3]) < 1e-6)), name


def test_adversarial_clouds_bite():
    """The preconditions the clouds are built for: many coordinates on which the float lattice and the exact one disagree, coordinates
    between 2^23 and 2^25 leaves from the origin, voxels of 1, 64 +- 1 and 100 000 points."""
    for leaf in (0.05, 0.1, 0.3):
        for sign in (1.0, -1.0):
            pts, vals = V.face_cloud(leaf, sign)
            assert V.disagrees(vals, leaf).all() and len(vals) >= 5
            assert V.disagrees(pts[:, :3], leaf).sum() >= 10000
    for leaf in (0.25, 0.5):                                    # exact leaves: the face points lie ON the faces, float and double agree
        pts, vals = V.face_cloud(leaf, 1.0, only_disagreeing=False)
        assert not V.disagrees(vals, leaf).any()
        assert np.any(np.floor(pts[:, 0] * np.float32(1 / leaf)) == pts[:, 0] * np.float32(1 / leaf))
    far = V.far_cloud(0.1, 24.0, -1.0)
    r = np.abs(far[:, :3].astype(np.float64)) / 0.1
    assert r.min() >= 2**23 and r.max() <= 2**25
    pts, leaf = V.awkward_clouds()["voxel_sizes"]
    assert sorted(collections.Counter(V.voxel_ref(pts, leaf).counts).keys()) == [1, 2, 63, 64, 65, 100_000]


def test_reference_on_small_hand_made_clouds():
    """The restatement itself, on cases small enough to state by hand."""
    pts = np.array([[0.05, 0.0, 0.0, 1.0], [0.15, 0.0, 0.0, 3.0], [0.06, 0.01, 0.02, 5.0], [np.nan, 0, 0, 9.0], [0.0, 0.0, 0.11, 7.0]], np.float32)
    r = V.voxel_ref(pts, 0.1)
    assert not r.unfiltered and len(r) == 3
    np.testing.assert_array_equal(r.voxel, [0, 1, 0, -1, 2])                        # div_b = (2, 1, 2): a z step is div_b0 * div_b1 = 2
    np.testing.assert_array_equal(r.members(0), [0, 2])
    np.testing.assert_allclose(r.mean64[0], [0.055, 0.005, 0.01, 3.0], rtol=1e-6)
    assert V.voxel_ref(np.full((3, 4), np.nan, np.float32), 0.1).mean64.shape == (0, 4)
    # the too-fine path returns the input, non-finite rows included
    tiny = np.array([[0, 0, 0, 1], [1e3, 1e3, 1e3, 2], [np.inf, 0, 0, 3]], np.float32)
    r = V.voxel_ref(tiny, 1e-4)
    assert r.unfiltered and len(r) == 3
    np.testing.assert_array_equal(r.mean64, tiny)


def test_too_fine_decision_is_pcls_near_int_max():
    """PCL's too-fine test, (int64)((max - min) * inv) + 1 per axis in float (voxel_grid_covariance_omp_impl.hpp:74-79), on boxes within a
    few voxels per axis of INT_MAX voxels: the oracle takes the unfiltered path exactly when the reference does.  The boxes include ones on
    which the lattice's floor count, floor(max * inv) - floor(min * inv) + 1, falls on the other side of INT_MAX, in both directions."""
    kinds = collections.Counter()
    for leaf, mn, mx in V.near_limit_boxes(2400, seed=11):
        pcl = V.pcl_too_fine(mn, mx, leaf)
        f = V.floor_axis_counts(mn, mx, leaf)
        kinds[(pcl, f[0] * f[1] * f[2] > V.INT_MAX)] += 1
        got, unfiltered = oracle.voxel_filter(np.stack([mn, mx]), leaf)
        assert unfiltered == pcl, (leaf, mn, mx)
        assert got.shape[0] == (2 if pcl else len(V.voxel_ref(np.stack([mn, mx]), leaf)))
    assert kinds[(True, False)] >= 3 and kinds[(False, True)] >= 100, kinds      # the cases where the two counts disagree
    assert kinds[(True, True)] >= 100 and kinds[(False, False)] >= 100, kinds


def test_the_1290_cube():
    """x in [0.05, 129.0], y and z in [0, 128.95] at leaf 0.1: 1290^3 voxels by PCL's count, 1291 * 1290^2 > INT_MAX by the floor count.
    PCL filters it; so must the oracle, with a few points that share voxels."""
    leaf, mn, mx = V.cube_1290()
    assert V.pcl_axis_counts(mn, mx, leaf) == [1290, 1290, 1290]
    assert V.floor_axis_counts(mn, mx, leaf) == [1291, 1290, 1290]
    assert not V.pcl_too_fine(mn, mx, leaf)
    pts = np.array([mn, mx, mn + np.float32(0.01), mx - np.float32(0.01), [64.0, 64.0, 64.0], [64.02, 64.03, 64.04]], np.float32)
    pts = np.concatenate([pts, np.arange(6, dtype=np.float32)[:, None]], 1)
    ref = V.voxel_ref(pts, leaf)
    got, unfiltered = oracle.voxel_filter(pts, leaf)
    assert not unfiltered and len(ref) == 4                # (the corners and their neighbours 0.01 inside: 0.06 shares 0.05's voxel, 128.99 not 129.0's)
    assert ref.ids.max() > V.INT_MAX                      # (PCL's int idx would wrap here: the oracle keeps the true order)
    np.testing.assert_array_equal(got, ref.sum32)
