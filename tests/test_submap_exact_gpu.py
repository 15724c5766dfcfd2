"""The key-frame store and sub-map assembly on the device (pcr_map_*, csrc/submap.hip) against the exact numpy restatement in
tests/submap_ref.py, point by point and voxel by voxel:

  - transformed bits: at a grid so fine that PCL's too-fine path returns its input, the sub-map IS the concatenation of the transformed key
    frames -- compared as uint32, row for row, with 1 .. 64 key frames (48 travel in the launch's arguments, 49 in a descriptor buffer);
  - membership and centroids: the row count is the reference's, row k lies in voxel ids[k] (floor(centroid * inv) - min_b, recomputed in
    float32), every averaged channel within one float32 ulp of the float64 mean of the reference's members;
  - on inputs that tests/test_submap_ref.py has qualified: key frames whose transformed points sit within a few ulps of voxel faces, several
    hundred of which a transform compiled WITH fused multiply-add would put into another voxel.

Every reference below is built with TRANSFORM.  With submap_ref.transform_contracted in its place the transformed-bits tests and the
face-membership tests fail: that is how these tests would meet a library built without -ffp-contract=off."""
import functools

import numpy as np
import pytest

import submap_ref as S
import voxel_ref as V
from simpleslam_amd import SubMap

pytestmark = pytest.mark.gpu

TRANSFORM = S.transform
FINE = 1e-4          # metres: any box of a few metres has more than INT_MAX voxels of it -- pcl::VoxelGrid returns the input
EVERYWHERE = (np.zeros(3), 1.0e3)


def _filled(clouds, poses):
    sm = SubMap()
    for c, T in zip(clouds, poses):
        sm.addKeyFrame(c, T)
    assert sm.keyframes() == len(clouds)
    return sm


def _ref(clouds, poses, selected, grid):
    return S.SubmapRef(clouds, poses, selected, grid, transform=TRANSFORM)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_exact(got, ref, what=""):
    """the unfiltered route: the transformed points bit for bit; the filtered one: row count, membership of every row, centroids to one ulp"""
    got = np.ascontiguousarray(got, np.float32)
    if ref.unfiltered:
        assert got.shape == ref.cat.shape, f"{what}: {got.shape} vs the concatenation's {ref.cat.shape}"
        bad = np.flatnonzero((_bits(got) != ref.bits()).any(1))
        assert len(bad) == 0, (f"{what}: {len(bad)} of {len(got)} transformed points differ in bits, the first: row {bad[0]} (key frame "
                               f"{ref.keyframe[bad[0]]}, point {ref.row[bad[0]]}): {got[bad[0]]!r} vs {ref.cat[bad[0]]!r}")
        return
    assert got.shape == (len(ref.ids), ref.stride), f"{what}: {got.shape[0]} rows vs {len(ref.ids)} voxels in the reference"
    if len(ref.ids) == 0:
        return
    assert np.isfinite(got[:, :3]).all(), what
    vid = S.voxel_of_rows(got, ref)
    bad = np.flatnonzero(vid != ref.ids)
    assert len(bad) == 0, f"{what}: {len(bad)} rows lie in another voxel than the reference's, the first: row {bad[0]}, voxel {vid[bad[0]]} vs {ref.ids[bad[0]]}"
    V.assert_matches_ref(got, ref.vox, max_ulp=1, what=what)


def _update_both_ways(clouds, poses, position, radius, grid):
    """pcr_map_update, and pcr_map_update_begin + pcr_map_wait on a second store: -> (sub-map, selection), the two byte-identical"""
    a, b = _filled(clouds, poses), _filled(clouds, poses)
    n = a.updateMap(position, radius=radius, grid_size=grid)
    b.updateMapBegin(position, radius=radius, grid_size=grid)
    assert b.wait() == n
    ga, gb = a.download(), b.download()
    assert ga.shape == gb.shape and ga.shape[0] == n == a.pointer()[1]
    np.testing.assert_array_equal(_bits(ga), _bits(gb))
    np.testing.assert_array_equal(a.submapIdx(), b.submapIdx())
    return ga, a.submapIdx()


# ---------------------------------------------------------------------------
# transformed bits
# ---------------------------------------------------------------------------
def _bits_store(n_kf, kind, stride):
    rng = np.random.default_rng([n_kf, 17])
    sizes = rng.integers(1, 60, n_kf)            # (a block of 256 output points straddles a handful of key frames)
    sizes[0] = 700
    if n_kf >= 48:
        sizes[20], sizes[21], sizes[22] = 2000, 1, 1
    return S.sized_keyframes(sizes, kind, seed=n_kf, stride=stride)


@pytest.mark.parametrize("kind", ["generic", "near_identity", "unrepresentable"])
@pytest.mark.parametrize("n_kf", [1, 3, 48, 49, 64])
def test_transformed_points_bit_for_bit(gpu, n_kf, kind):
    """1, 3, 48, 49 and 64 selected key frames under generic rotations, rotations of 1e-7 .. 1e-3 rad, and poses whose doubles no float holds
    (the cast): at a 0.1 mm grid the box of every one of these stores is too fine for pcl::VoxelGrid, so the sub-map is the concatenation."""
    stride = 8 if n_kf in (3, 49) else 4
    clouds, poses = _bits_store(n_kf, kind, stride)
    ref = _ref(clouds, poses, S.select_radius(poses, *EVERYWHERE), FINE)
    assert ref.unfiltered and len(ref.selected) == n_kf and ref.cat.shape[1] == stride
    sm = _filled(clouds, poses)
    n = sm.updateMap(EVERYWHERE[0], radius=EVERYWHERE[1], grid_size=FINE)
    np.testing.assert_array_equal(sm.submapIdx(), ref.selected)
    assert n == ref.cat.shape[0]
    _check_exact(sm.download(), ref, what=f"{n_kf} key frames, {kind}")


# ---------------------------------------------------------------------------
# membership and centroids
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _membership_fixture(name, grid):
    if name == "faces":
        clouds, poses = S.face_fixture(grid, seed=int(grid * 10))
        return clouds, poses, np.zeros(3), 50.0
    clouds, poses = S.trajectory_keyframes()
    return clouds, poses, poses[3][:3, 3].copy(), 8.0


@pytest.mark.parametrize("stride", [4, 8])
@pytest.mark.parametrize("grid", [0.4, 0.5])
@pytest.mark.parametrize("name", ["faces", "trajectory"])
def test_membership_and_centroids(gpu, name, grid, stride):
    """The face fixtures (qualified in tests/test_submap_ref.py: hundreds of their points change voxel under a contracted transform, and a centre
    point in every touched voxel turns that into centroids that move by a good part of the leaf) and the `keyframes` trajectory of
    tests/test_submap_gpu.py, at 16- and 32-byte points."""
    clouds, poses, position, radius = _membership_fixture(name, grid)
    clouds = [S.widen(c, stride) for c in clouds]
    ref = _ref(clouds, poses, S.select_radius(poses, position, radius), grid)
    assert not ref.unfiltered and len(ref.selected) >= 5
    sm = _filled(clouds, poses)
    n = sm.updateMap(position, radius=radius, grid_size=grid)
    np.testing.assert_array_equal(sm.submapIdx(), ref.selected)
    assert n == len(ref.ids)
    _check_exact(sm.download(), ref, what=f"{name} grid {grid} stride {stride}")


# ---------------------------------------------------------------------------
# 48 / 49 key frames: descriptors in the launch's arguments, descriptors in a buffer
# ---------------------------------------------------------------------------
def test_48_and_49_keyframes_of_one_store(gpu):
    """One store, one position: a radius of 8 m selects 48 key frames (submap_transform_pack_kernel), 9.5 m a 49th (submap_transform_kernel) whose
    points fall into voxels the 48 already occupy.  Both meet the reference -- bits at the fine grid, membership and centroids at 0.4 and 0.5 --
    and the 48 key frames' transformed points are the same bits in both runs."""
    clouds, poses, position, r48, r49 = S.boundary_store()
    sm = _filled(clouds, poses)
    fine = {}
    for want, radius in ((48, r48), (49, r49)):
        sel = S.select_radius(poses, position, radius)
        assert len(sel) == want and all(len(clouds[i]) for i in sel)
        ref = _ref(clouds, poses, sel, FINE)
        assert ref.unfiltered
        assert sm.updateMap(position, radius=radius, grid_size=FINE) == ref.cat.shape[0]
        np.testing.assert_array_equal(sm.submapIdx(), sel)
        fine[want] = sm.download()
        _check_exact(fine[want], ref, what=f"{want} key frames, fine grid")
    n48 = fine[48].shape[0]
    assert fine[49].shape[0] == n48 + len(clouds[48])
    np.testing.assert_array_equal(_bits(fine[49][:n48]), _bits(fine[48]))
    for grid in (0.4, 0.5):
        refs = {}
        for want, radius in ((49, r49), (48, r48)):
            refs[want] = _ref(clouds, poses, S.select_radius(poses, position, radius), grid)
            assert sm.updateMap(position, radius=radius, grid_size=grid) == len(refs[want].ids)
            _check_exact(sm.download(), refs[want], what=f"{want} key frames, grid {grid}")
        # the 49th key frame opens no voxel: it only adds members to occupied ones
        np.testing.assert_array_equal(refs[49].ids, refs[48].ids)
        assert refs[49].vox.counts.sum() == refs[48].vox.counts.sum() + len(clouds[48])


def test_49_selected_of_which_one_is_empty(gpu):
    """49 key frames selected, one of them empty: 48 descriptors -- the argument-carried kernel -- and indices that still name all 49."""
    clouds, poses, position, _, r49 = S.boundary_store()
    clouds = list(clouds)
    clouds[17] = np.zeros((0, 4), np.float32)
    for grid in (FINE, 0.4):
        got, sel = _update_both_ways(clouds, poses, position, r49, grid)
        np.testing.assert_array_equal(sel, np.arange(49))
        _check_exact(got, _ref(clouds, poses, sel, grid), what=f"49 selected, key frame 17 empty, grid {grid}")


# ---------------------------------------------------------------------------
# ragged concatenations: the per-point search for the owning key frame
# ---------------------------------------------------------------------------
RAGGED = {
    "0_1_255_256_257": [0, 1, 255, 256, 257],
    "257_0_1_256_255_1_1": [257, 0, 1, 256, 255, 1, 1],
    "empty_first": [0, 5, 7],
    "empty_last": [5, 7, 0],
    "empty_between": [5, 0, 7],
    "two_adjacent_empty": [5, 0, 0, 7],
    "one_point_in_all": [0, 1, 0],
    "only_empty": [0, 0, 0],
    "ones": [1] * 40,
}


@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_concatenations(gpu, name):
    """Empty key frames before, after and between occupied ones, 1-point key frames, sizes either side of a block: through pcr_map_update and
    through pcr_map_update_begin / pcr_map_wait, byte-identical, and exact against the reference on both routes -- transformed bits at the fine
    grid (a selection of one point has a box of one voxel at any grid: it goes through the filter, whose mean of one point is the point),
    membership and centroids at 0.4."""
    sizes = RAGGED[name]
    clouds, poses = S.sized_keyframes(sizes, "generic", seed=len(sizes) + sum(sizes))
    for grid in (FINE, 0.4):
        got, sel = _update_both_ways(clouds, poses, *EVERYWHERE, grid)
        np.testing.assert_array_equal(sel, np.arange(len(sizes)))            # an empty key frame is still a selected one (mSubmapIdx)
        ref = _ref(clouds, poses, sel, grid)
        assert ref.unfiltered == (grid == FINE and sum(sizes) > 1), name
        if sum(sizes) <= 1:
            assert got.shape[0] == sum(sizes)
            np.testing.assert_array_equal(_bits(got), ref.bits())
        _check_exact(got, ref, what=f"{name} grid {grid}")


# ---------------------------------------------------------------------------
# the other entry points
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_store():
    """12 key frames of 30 .. 400 points along a line, 1.5 m apart, generic rotations; key frame 5 empty"""
    sizes = [120, 30, 400, 77, 256, 0, 257, 90, 64, 300, 33, 150]
    clouds, poses = S.sized_keyframes(sizes, "generic", seed=12)
    for j, T in enumerate(poses):
        T[:3, 3] = [1.5 * j, 0.3 * (j % 3), -0.2 * (j % 2)]
    return clouds, poses


@pytest.mark.parametrize("grid", [FINE, 0.4])
def test_update_window(gpu, grid):
    clouds, poses = _small_store()
    sm = _filled(clouds, poses)
    for key, num in ((4, 2), (0, 2), (11, 3), (5, 0)):
        sel = S.select_window(len(clouds), key, num)
        ref = _ref(clouds, poses, sel, grid)
        n = sm.loopFindNearKeyframes(key, num, grid_size=grid)
        np.testing.assert_array_equal(sm.submapIdx(), sel)
        assert n == len(ref)
        _check_exact(sm.download(), ref, what=f"window {key} +- {num} grid {grid}")


@pytest.mark.parametrize("grid", [FINE, 0.4])
def test_update_all(gpu, grid):
    clouds, poses = _small_store()
    sm = _filled(clouds, poses)
    ref = _ref(clouds, poses, S.select_all(len(clouds)), grid)
    assert sm.updateAll(grid_size=grid) == len(ref)
    np.testing.assert_array_equal(sm.submapIdx(), ref.selected)
    _check_exact(sm.download(), ref, what=f"all, grid {grid}")


@pytest.mark.parametrize("grid", [FINE, 0.4])
def test_a_views_update(gpu, grid):
    """a view's sub-map over the parent's key frames, while the parent holds another selection: each exact, neither disturbed by the other"""
    clouds, poses = _small_store()
    sm = _filled(clouds, poses)
    view = sm.view()
    p_parent, p_view = poses[2][:3, 3], poses[9][:3, 3]
    ref_parent = _ref(clouds, poses, S.select_radius(poses, p_parent, 4.0), grid)
    ref_view = _ref(clouds, poses, S.select_radius(poses, p_view, 3.5), grid)
    assert len(ref_parent.selected) >= 3 and len(ref_view.selected) >= 3 and set(ref_parent.selected) != set(ref_view.selected)
    assert sm.updateMap(p_parent, radius=4.0, grid_size=grid) == len(ref_parent)
    view.updateMapBegin(p_view, radius=3.5, grid_size=grid)
    assert view.wait() == len(ref_view)
    np.testing.assert_array_equal(view.submapIdx(), ref_view.selected)
    np.testing.assert_array_equal(sm.submapIdx(), ref_parent.selected)
    _check_exact(view.download(), ref_view, what=f"view, grid {grid}")
    _check_exact(sm.download(), ref_parent, what=f"parent beside a view, grid {grid}")


@pytest.mark.parametrize("grid", [FINE, 0.4])
def test_update_after_set_poses(gpu, grid):
    """new poses for key frames 3 .. 8 -- one moved out of the radius, one into it, the rest turned: the next update selects by the new
    translations and transforms by the new poses cast to float"""
    clouds, poses = _small_store()
    far = np.array([0.0, 40.0, 0.0])
    start = [T.copy() for T in poses]
    start[6][:3, 3] += far
    sm = _filled(clouds, start)
    position, radius = poses[5][:3, 3], 5.0
    before = _ref(clouds, start, S.select_radius(start, position, radius), grid)
    assert sm.updateMap(position, radius=radius, grid_size=grid) == len(before)
    _check_exact(sm.download(), before, what="before the poses change")
    new = [T.copy() for T in start]
    new[6] = poses[6].copy()
    new[4][:3, 3] += far
    for j, kind in ((3, "near_identity"), (7, "unrepresentable"), (8, "generic")):
        new[j][:3, :3] = S.poses_of_kind(kind, 1, seed=60 + j)[0][:3, :3] @ new[j][:3, :3]
    new[7][:3, 3] += 1.0 / 3.0
    sm.setPoses(3, np.array(new[3:9]))
    after = _ref(clouds, new, S.select_radius(new, position, radius), grid)
    assert 6 in after.selected and 6 not in before.selected and 4 in before.selected and 4 not in after.selected
    assert sm.updateMap(position, radius=radius, grid_size=grid) == len(after)
    np.testing.assert_array_equal(sm.submapIdx(), after.selected)
    _check_exact(sm.download(), after, what=f"after set_poses, grid {grid}")


@pytest.mark.parametrize("grid", [FINE, 0.4])
def test_downsample_keyframes_then_update(gpu, grid):
    """pcr_map_downsample_keyframes(first = 2, 3.0): every later key frame becomes the filter's output for its own cloud IN ITS OWN FRAME -- held
    to the voxel reference's bars (rows, one ulp of the float64 mean); the earlier ones keep their bytes.  The update that follows is exact
    against the reference assembled from the key frames as they are now stored."""
    clouds, poses = _small_store()
    sm = _filled(clouds, poses)
    want = S.downsampled(clouds, 2, 3.0)
    assert sum(len(c) for c in want) < 0.8 * sum(len(c) for c in clouds)
    assert sm.downSampleKeyFrames(2, 3.0) == sum(len(c) for c in want)
    stored = []
    for i, c in enumerate(clouds):
        got, T = sm.keyFrame(i)
        np.testing.assert_array_equal(T, poses[i])
        if i < 2:
            np.testing.assert_array_equal(_bits(got), _bits(c))
        elif len(c):
            own = V.VoxelRef(c, 3.0)
            assert not own.unfiltered
            V.assert_matches_ref(got, own, max_ulp=1, what=f"key frame {i} filtered in its own frame")
        assert got.shape == (len(want[i]), 4)
        stored.append(got)
    ref = _ref(stored, poses, S.select_all(len(clouds)), grid)
    assert sm.updateAll(grid_size=grid) == len(ref)
    _check_exact(sm.download(), ref, what=f"update after downsample_keyframes, grid {grid}")


def test_non_finite_rows_reach_no_voxel(gpu):
    """NaN and +-Inf coordinates in two key frames: those points reach no voxel, every other point reaches its own, the row count is the reference's"""
    clouds, poses = _small_store()
    clouds = [c.copy() for c in clouds]
    clouds[2][[0, 17, 255, 256, 399], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    clouds[4][[3, 100], [2, 0]] = [np.nan, -np.inf]
    clean = [c[np.isfinite(c[:, :3]).all(1)] for c in clouds]
    sm = _filled(clouds, poses)
    for grid in (0.4, 0.5):
        ref = _ref(clouds, poses, S.select_all(len(clouds)), grid)
        assert (~ref.vox.finite).sum() == 7 and not ref.unfiltered
        assert sm.updateAll(grid_size=grid) == len(ref.ids)
        got = sm.download()
        _check_exact(got, ref, what=f"non-finite rows, grid {grid}")
        # ... which is the sub-map of the store without those points
        without = _ref(clean, poses, S.select_all(len(clouds)), grid)
        np.testing.assert_array_equal(without.ids, ref.ids)
        np.testing.assert_array_equal(_bits(without.mean64), _bits(ref.mean64))
