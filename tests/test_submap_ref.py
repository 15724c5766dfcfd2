"""CPU tests (no GPU): tests/submap_ref.py -- the plain numpy restatement of the sub-map assembly -- pinned against the oracle
(oracle/submap_oracle.c), and the inputs of tests/test_submap_exact_gpu.py qualified: the face fixtures must be ones on which a contracted
transform (fused multiply-add) puts points into other voxels, or the device tests that use them would prove nothing about contraction."""
import numpy as np
import pytest

import oracle
import submap_ref as S
import voxel_ref as V


def _radius_edge():
    """poses at exactly `radius` from the position, one float64 step inside it and one outside, along an axis and askew"""
    pos, r = np.zeros(3), 8.0          # (the origin: position - translation is then the offset itself, the last bit included)
    offs = [[0, 0, 0], [3, 0, 0], [r, 0, 0], [np.nextafter(r, 0.0), 0, 0], [np.nextafter(r, 9.0), 0, 0], [0, -r, 0], [0, 0, np.nextafter(r, 0.0)],
            [0, 4.8, 6.4], [4.0, 4.0, np.sqrt(32.0)], [-4.0, 4.0, np.nextafter(np.sqrt(32.0), 0.0)], [100, 0, 0]]
    poses = [S.pose([0.1 * j, 0.2, -0.3], pos + np.array(o, np.float64)) for j, o in enumerate(offs)]
    clouds = [S.random_cloud(5 + j, 300 + j) for j in range(len(offs))]
    return clouds, poses, pos, r


def _cases():
    """name -> (clouds, poses, position, radius, grid): the selections and assemblies the GPU tests run"""
    out = {}
    for grid in (0.4, 0.5):
        c, p = S.face_fixture(grid, seed=int(grid * 10))
        out[f"faces_{grid}"] = (c, p, np.zeros(3), 50.0, grid)
    c, p = S.trajectory_keyframes()
    for k, (j, radius, far) in enumerate(((3, 8.0, 0.0), (10, 3.0, 0.0), (0, 8.0, 100.0))):
        out[f"trajectory_{k}"] = (c, p, p[j][:3, 3] + far, radius, 0.4)
    c, p, pos, r48, r49 = S.boundary_store()
    out["boundary_48"] = (c, p, pos, r48, 0.4)
    out["boundary_49"] = (c, p, pos, r49, 0.5)
    c, p, pos, r = _radius_edge()
    out["radius_edge"] = (c, p, pos, r, 0.4)
    c, p = S.sized_keyframes([0, 1, 255, 0, 0, 256, 257, 0], "generic", seed=7)
    out["ragged"] = (c, p, np.zeros(3), 50.0, 0.4)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_selection_and_rows_equal_the_oracles(name):
    """The same key frames, the same number of rows, and every oracle centroid (float32 sums in input order) within the float-accumulation bound
    of tests/test_voxel_ref.py -- 64 ulps or 1e-6 -- of the reference's float64 mean."""
    clouds, poses, pos, radius, grid = CASES[name]
    ref = S.assemble(clouds, poses, pos, radius, grid)
    got, sel = oracle.submap_assemble(clouds, poses, pos, radius, grid)
    np.testing.assert_array_equal(sel, ref.selected)
    assert got.shape[0] == len(ref), name
    if len(ref):
        d = V.ulp_distance(got[:, :3], ref.mean64[:, :3])
        assert np.all((d <= 64) | (np.abs(got[:, :3] - ref.mean64[:, :3]) < 1e-6)), name
        np.testing.assert_array_equal(got, ref.vox.sum32)       # (and the oracle's transform is the reference's, bit for bit: equal sums of equal points)


def test_radius_edge_is_strict_in_float64():
    clouds, poses, pos, r = _radius_edge()
    sel = S.select_radius(poses, pos, r)
    assert 2 not in sel and 5 not in sel and 4 not in sel and 10 not in sel        # at exactly the radius, beyond it
    assert {0, 1, 3, 6} <= set(sel.tolist())                                        # nextafter(radius, 0) is in
    np.testing.assert_array_equal(sel, np.sort(sel))
    np.testing.assert_array_equal(S.select_window(14, 3, 2), [1, 2, 3, 4, 5])
    np.testing.assert_array_equal(S.select_window(14, 0, 2), [0, 1, 2])
    np.testing.assert_array_equal(S.select_window(14, 13, 3), [10, 11, 12, 13])
    np.testing.assert_array_equal(S.select_window(3, 7, 2), [])
    np.testing.assert_array_equal(S.select_all(4), [0, 1, 2, 3])


def test_transform_rounds_after_every_operation():
    """the float32 expression against the same steps taken in float64 and rounded by hand, and the cast of the pose"""
    T = S.poses_of_kind("unrepresentable", 1, seed=1)[0]
    R, t = S.pose_f32(T)
    assert R.dtype == t.dtype == np.float32 and not np.array_equal(R.astype(np.float64), T[:3, :3])
    pts = S.random_cloud(500, 11)
    got = S.transform(pts, T)
    f = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    x, y, z = (pts[:, c].astype(np.float64) for c in range(3))
    for r in range(3):
        R64, t64 = R.astype(np.float64), t.astype(np.float64)
        want = f(f(f(f(R64[r, 0] * x) + f(R64[r, 1] * y)) + f(R64[r, 2] * z)) + t64[r])      # (products of floats are exact in float64: one rounding each)
        np.testing.assert_array_equal(got[:, r].astype(np.float64), want)
    np.testing.assert_array_equal(got[:, 3], pts[:, 3])
    # a pose of the identity moves nothing, under either variant
    I = np.eye(4)
    np.testing.assert_array_equal(S.transform(pts, I), pts)
    np.testing.assert_array_equal(S.transform_contracted(pts, I), pts)


@pytest.mark.parametrize("grid", [0.4, 0.5])
def test_face_fixtures_are_sensitive_to_contraction(grid):
    """At least 32 points of each face fixture fall into another voxel under the contracted transform -- a condition on the INPUTS."""
    clouds, poses = S.face_fixture(grid, seed=int(grid * 10))
    n_flip, n_bits, n_all = S.flips(clouds, poses, grid)
    print(f"face fixture grid {grid}: {n_flip} of {n_all // 3} points change voxel under contraction, {n_bits} of {n_all} coordinates differ in bits")
    assert n_flip >= 32
    # and the centre points make a flip visible: every touched voxel is occupied by a point of the last key frame under either variant
    exact = S.assemble(clouds, poses, np.zeros(3), 50.0, grid)
    fused = S.assemble(clouds, poses, np.zeros(3), 50.0, grid, transform=S.transform_contracted)
    assert len(exact) == len(fused)
    moved = V.ulp_distance(exact.mean64[:, :3], fused.mean64[:, :3]).max(1) > 1000
    print(f"    {int(moved.sum())} of {len(exact)} centroids move by more than 1000 ulps")
    assert moved.sum() >= 32


def test_rotated_poses_differ_in_bits_under_contraction():
    """Across the rotated-pose fixtures together at least 10 % of the transformed coordinates differ in bits between the two variants."""
    n_bits = n_all = 0
    for kind in ("generic", "near_identity", "unrepresentable"):
        clouds, poses = S.sized_keyframes([300] * 8, kind, seed=21)
        _, b, a = S.flips(clouds, poses, 0.4)
        print(f"{kind}: {b} of {a} coordinates differ in bits ({100.0 * b / a:.1f} %)")
        n_bits += b; n_all += a
    for grid in (0.4, 0.5):
        clouds, poses = S.face_fixture(grid, seed=int(grid * 10))
        _, b, a = S.flips(clouds[:-1], poses[:-1], grid)
        print(f"faces {grid}: {b} of {a} coordinates differ in bits ({100.0 * b / a:.1f} %)")
        n_bits += b; n_all += a
    print(f"together: {n_bits} of {n_all} ({100.0 * n_bits / n_all:.1f} %)")
    assert n_bits >= 0.10 * n_all


@pytest.mark.parametrize("name", ["faces_0.4", "trajectory_0", "ragged"])
def test_result_does_not_depend_on_the_keyframe_order(name):
    """the selection reversed and shuffled: the same voxels, the same members per voxel (as sets of (key frame, row)), the same means"""
    clouds, poses, pos, radius, grid = CASES[name]
    ref = S.assemble(clouds, poses, pos, radius, grid)
    sets = ref.voxel_sets()
    rng = np.random.default_rng(4)
    for order in (ref.selected[::-1], rng.permutation(ref.selected)):
        other = S.SubmapRef(clouds, poses, order, grid)
        np.testing.assert_array_equal(other.ids, ref.ids)
        assert other.voxel_sets() == sets
        assert V.ulp_distance(other.mean64, ref.mean64).max() <= 1       # (float64 sums in another order: the same float32 but for a tie)
    assert sum(len(s) for s in sets.values()) == int(ref.vox.finite.sum())


def test_reference_on_a_hand_made_store():
    """two key frames, three points, stated by hand"""
    clouds = [np.array([[1.0, 0.0, 0.0, 5.0], [0.0, 1.0, 0.0, 7.0]], np.float32), np.array([[0.0, 0.0, 0.0, 9.0]], np.float32), np.zeros((0, 4), np.float32)]
    Rz = S.pose([0, 0, np.pi / 2], [10.0, 0.0, 0.0])                       # x -> y, y -> -x
    poses = [Rz, S.pose([0, 0, 0], [10.05, 1.05, 0.0]), np.eye(4)]
    ref = S.assemble(clouds, poses, [10.0, 0.0, 0.0], 2.0, 0.5)
    np.testing.assert_array_equal(ref.selected, [0, 1])                    # (the third, at 10 m, is out)
    np.testing.assert_allclose(ref.cat[:, :3], [[10, 1, 0], [9, 0, 0], [10.05, 1.05, 0]], atol=1e-6)
    np.testing.assert_array_equal(ref.keyframe, [0, 0, 1])
    np.testing.assert_array_equal(ref.row, [0, 1, 0])
    assert len(ref) == 2 and ref.voxel[0] == ref.voxel[2] != ref.voxel[1]
    np.testing.assert_allclose(ref.mean64[ref.ids.tolist().index(ref.voxel[0])], [10.025, 1.025, 0.0, 7.0], atol=1e-6)
    # an unfiltered grid: the sub-map is the concatenation
    fine = S.assemble(clouds, poses, [10.0, 0.0, 0.0], 2.0, 1e-7)
    assert fine.unfiltered and len(fine) == 3
    np.testing.assert_array_equal(fine.mean64, fine.cat)
