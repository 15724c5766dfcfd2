"""pcl::VoxelGrid on the device (pcr_voxel_filter and the sub-map assembly) against the exact numpy restatement in tests/voxel_ref.py, at
the inputs where a voxel filter goes wrong: points on voxel faces and 1-2 ulps either side, coordinates 2^23-2^25 leaves from the origin,
duplicated and lattice-quantised points, non-finite rows, voxels of one wave +- 1 and of 100 000 points, every point layout, the index's
box hints, boxes next to PCL's INT_MAX limit and boxes whose padded index would exceed the dense table's.

Every check: the same number of rows as the reference, and every averaged channel within one float32 ulp of the reference's float64 mean.
A point put into the wrong voxel moves a centroid by far more than an ulp (the face clouds also hold a point at the centre of every voxel
they touch), so this makes membership exact."""
import gc

import numpy as np
import pytest

import oracle
import voxel_ref as V
from simpleslam_amd import LoamRegister, SubMap, synth

pytestmark = pytest.mark.gpu


def _filter(pts, leaf, reg=None):
    return (reg or LoamRegister()).voxelDownSample(pts, leaf)


@pytest.mark.parametrize("leaf", [0.05, 0.1, 0.3, 0.25, 0.5])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_points_on_and_next_to_voxel_faces(gpu, leaf, sign):
    exact = leaf in (0.25, 0.5)
    pts, vals = V.face_cloud(leaf, sign, seed=int(leaf * 1000) + (sign > 0), only_disagreeing=not exact)
    if exact:       # an exact leaf: the face points lie ON the faces (x * inv is exact), float and double agree
        assert not V.disagrees(vals, leaf).any() and np.any(np.floor(pts[:, 0] / np.float32(leaf)) == pts[:, 0] / np.float32(leaf))
    else:           # only coordinates on which floor(float(x) * inv_f) != floor(double(x) / double(leaf)), and many of them
        assert V.disagrees(vals, leaf).all() and V.disagrees(pts[:, :3], leaf).sum() >= 10000
    V.assert_matches_ref(_filter(pts, leaf), V.voxel_ref(pts, leaf), what=f"faces leaf {leaf} sign {sign}")


@pytest.mark.parametrize("leaf,log2_ratio,sign", [(0.05, 23.1, 1.0), (0.05, 24.5, -1.0), (0.1, 23.5, -1.0), (0.1, 24.0, 1.0),
                                                  (0.3, 24.9, 1.0), (0.25, 24.2, -1.0)])
def test_far_from_the_origin(gpu, leaf, log2_ratio, sign):
    """UTM-like coordinates at a small leaf: |x| / leaf between 2^23 and 2^25, where float32 holds only every second or fourth voxel face."""
    pts = V.far_cloud(leaf, log2_ratio, sign, seed=int(log2_ratio * 10))
    r = np.abs(pts[:, :3].astype(np.float64)) / leaf
    assert r.min() >= 2**23 and r.max() <= 2**25
    V.assert_matches_ref(_filter(pts, leaf), V.voxel_ref(pts, leaf), what=f"far {leaf} 2^{log2_ratio}")


@pytest.mark.parametrize("name", list(V.awkward_clouds().keys()))
def test_awkward_content_and_voxel_sizes(gpu, name):
    """duplicated points, lattice-quantised clouds, NaN / +-Inf rows in each axis, voxels of 1, 63, 64, 65 and 100 000 points"""
    pts, leaf = V.awkward_clouds()[name]
    ref = V.voxel_ref(pts, leaf)
    if name == "voxel_sizes":
        assert set(ref.counts) == {1, 2, 63, 64, 65, 100_000}
    if "inf" in name or "nan" in name:
        assert (~ref.finite).sum() == 97
    V.assert_matches_ref(_filter(pts, leaf), ref, what=name)


@pytest.mark.parametrize("stride", [3, 4, 5, 6, 7, 8])
def test_point_layouts_host_device_and_in_two_halves(gpu, stride):
    """12- to 32-byte points, from host memory, from device memory and through pcr_voxel_filter_begin / _end: the same voxels each way."""
    import torch
    src, _ = V.face_cloud(0.1, -1.0, seed=stride)
    pts = np.random.default_rng(stride).random((src.shape[0], stride), dtype=np.float32) * 7      # further floats: ignored, zero in the output
    pts[:, :3] = src[:, :3]
    ic = V.intensity_column(stride)
    if ic is not None:
        pts[:, ic] = src[:, 3]
    ref = V.voxel_ref(pts, 0.1)
    reg = LoamRegister()
    V.assert_matches_ref(reg.voxelDownSample(pts, 0.1), ref, what=f"host stride {stride}")
    d = torch.from_numpy(pts).cuda()
    V.assert_matches_ref(reg.voxelDownSample(d, 0.1).cpu().numpy(), ref, what=f"device stride {stride}")
    tok = reg.voxelDownSampleBegin(d, 0.1)
    V.assert_matches_ref(reg.voxelDownSampleEnd(tok).cpu().numpy(), ref, what=f"begin/end stride {stride}")


def test_box_hints_just_inside_and_outside_the_padded_box(gpu):
    """One handle through clouds placed just inside and just outside the previous call's padded box (16 cells in x and y, 4 in z, around the
    box of the last fresh build): the reused header must never change a result.  Every result equals the reference and a fresh handle's."""
    leaf = 0.1
    base, _ = V.face_cloud(leaf, 1.0, n=8000, seed=5)
    reg = LoamRegister()
    moves = [(0, 0, 0), (15.5, 0, 0), (16.5, 0, 0), (0, 0, 0), (0, -15.5, 0), (0, -16.5, 0), (0, 0, 3.5), (0, 0, 4.5), (0, 0, -4.5),
             (-16.5, 15.5, 3.5), (0, 0, 0), (0.5, 0.5, 0.5)]
    for m in moves:
        pts = base.copy()
        pts[:, :3] += (np.array(m, np.float64) * leaf).astype(np.float32)
        ref = V.voxel_ref(pts, leaf)
        a = reg.voxelDownSample(pts, leaf)
        b = _filter(pts, leaf)
        V.assert_matches_ref(a, ref, what=f"hinted handle after move {m}")
        V.assert_matches_ref(b, ref, what=f"fresh handle, move {m}")
        assert V.ulp_distance(a, b).max() <= 1


def _transform_f32(pts, T):
    """pcp::transformPointCloud with the pose cast to float, ((r0 x + r1 y) + r2 z) + t, as oracle/submap_oracle.c forms it"""
    R = np.asarray(T, np.float64)[:3, :3].astype(np.float32)
    t = np.asarray(T, np.float64)[:3, 3].astype(np.float32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = pts.copy()
    for r in range(3):
        out[:, r] = ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r]
    return out


def _face_keyframes():
    kfs = []
    for j, (leaf, sign) in enumerate([(0.4, 1.0), (0.4, -1.0), (0.1, 1.0), (0.3, -1.0), (0.4, 1.0)]):
        pts, _ = V.face_cloud(leaf, sign, n=4000, seed=40 + j)
        T = np.eye(4)
        if j % 2:           # a pose with a rotation: the transformed points land anywhere; without one, the faces stay faces of the 0.4 lattice
            T[:3, :3] = synth.perturb(np.eye(4), j, trans=0.0, rot_deg=3.0)[:3, :3]
        T[:3, 3] = [0.4 * j, -0.8 * j, 0.0]
        kfs.append((pts, T))
    return kfs


def test_submap_assembly_of_face_clouds(gpu):
    """The face clouds as key frames through SubMap.updateMap and through pcr_map_update_begin + pcr_scan2map_submap: the sub-map equals
    voxel_ref of the concatenation that oracle.submap_assemble transforms."""
    kfs = _face_keyframes()
    centre, radius, grid = np.zeros(3), 50.0, 0.4
    cat = np.concatenate([_transform_f32(c, T) for c, T in kfs])
    ref = V.voxel_ref(cat, grid)
    ora, sel = oracle.submap_assemble([c for c, _ in kfs], [T for _, T in kfs], centre, radius, grid)
    assert len(sel) == len(kfs) and ora.shape[0] == len(ref)
    np.testing.assert_array_equal(ora, ref.sum32)                      # (the oracle's own transform is the one restated above)
    sm = SubMap()
    for c, T in kfs:
        sm.addKeyFrame(c, T)
    assert sm.updateMap(centre, radius=radius, grid_size=grid) == len(ref)
    V.assert_matches_ref(sm.download(), ref, what="updateMap")
    # queued, then collected by the registration that asks for it
    world, _ = synth.make_map(20_000, seed=3)
    scan, T = synth.make_scan(world, 0, seed=3, beams=16, azimuths=256)
    sm2 = SubMap()
    for c, Tk in kfs:
        sm2.addKeyFrame(c, Tk)
    sm2.updateMapBegin(centre, radius=radius, grid_size=grid)
    reg = LoamRegister()
    pose = np.eye(4)
    reg.scan2MapSubmap(reg.voxelDownSample(scan, 0.4), sm2, pose)
    V.assert_matches_ref(sm2.download(), ref, what="updateMapBegin + scan2MapSubmap")


def test_boxes_on_pcls_too_fine_side_come_back_unfiltered(gpu):
    """Boxes within a few voxels per axis of INT_MAX voxels that PCL's count puts over the limit -- among them ones that the lattice's floor
    count would let through -- return the input unchanged, a NaN row included.  Nothing is indexed for them."""
    reg = LoamRegister()
    n_split = n = 0
    for leaf, mn, mx in V.near_limit_boxes(900, seed=23):
        if not V.pcl_too_fine(mn, mx, leaf):
            continue
        f = V.floor_axis_counts(mn, mx, leaf)
        split = f[0] * f[1] * f[2] <= V.INT_MAX
        if not split and n >= 40:
            continue
        pts = np.array([[*mn, 1.0], [np.nan, 0, 0, 2.0], [*mx, 3.0]], np.float32)
        got = reg.voxelDownSample(pts, leaf)
        np.testing.assert_array_equal(got, pts)
        n += 1; n_split += split
    assert n >= 40 and n_split >= 1, (n, n_split)


def _peak_filter(pts, leaf):
    """the filter on a handle of its own, destroyed right after; -> (output, device memory the call held at its peak, in bytes)"""
    import torch
    free0, _ = torch.cuda.mem_get_info()
    reg = LoamRegister()
    got = reg.voxelDownSample(pts, leaf)
    free1, _ = torch.cuda.mem_get_info()
    reg.close()
    del reg
    gc.collect()
    return got, free0 - free1


def test_the_1290_cube_just_under_the_limit_is_filtered(gpu):
    """x in [0.05, 129.0], y and z in [0, 128.95] at leaf 0.1: PCL counts 1290^3 = 2 146 689 000 voxels and filters; the floor count,
    1291 * 1290^2, is over INT_MAX.  The device must filter it, with a few points sharing voxels.

    This builds the filter's dense table over the whole padded box -- about 2.27e9 cells, some 27 GB of cell counters and starts -- so it runs
    once, on a handle of its own that is destroyed right after."""
    leaf, mn, mx = V.cube_1290()
    pts = np.array([[*mn, 1], [*mx, 2], [*(mn + np.float32(0.01)), 3], [*(mx - np.float32(0.01)), 4], [64.0, 64.0, 64.0, 5],
                    [64.02, 64.03, 64.04, 6], [np.inf, 1, 1, 7]], np.float32)
    ref = V.voxel_ref(pts, leaf)
    assert not ref.unfiltered and len(ref) == 4
    got, peak = _peak_filter(pts, leaf)
    print(f"1290^3 cube: {peak / 1e9:.1f} GB of device memory held by the filter's handle")
    V.assert_matches_ref(got, ref, what="1290^3 cube")


@pytest.mark.parametrize("shape", ["flat_2km_0.05", "line_0.01"])
def test_flat_and_line_clouds_whose_padded_box_exceeds_the_table(gpu, shape):
    """Clouds that PCL filters but whose box, padded by the index's margins (16 cells in x and y, 4 in z), would need more than the dense
    table's 4e9 cells: a flat cloud 2 km across at a 0.05 m leaf (40 001^2 voxels; 40 033^2 x 9 padded) and a line 1.5e7 voxels long
    (padded: x 33 x 9 = 4.5e9).  They must be filtered and match the reference."""
    rng = np.random.default_rng(8)
    if shape.startswith("flat"):
        leaf, n = 0.05, 30000
        xy = rng.random((n, 2)) * 2000.0 - 1000.0
        pts = np.zeros((n + 6, 4), np.float32)
        pts[:n, :2] = xy
        pts[n:, :2] = [[-1000, -1000], [1000, 1000], [-1000, 1000], [1000, -1000], [3.01, 4.01], [3.02, 4.03]]
        pts[:, 2] = 0.02
    else:
        leaf, n = 0.01, 30000
        pts = np.zeros((n + 4, 4), np.float32)
        pts[:n, 0] = rng.random(n) * 1.5e5
        pts[n:, 0] = [0.0, 1.5e5 - 0.005, 7.001, 7.002]
        pts[:, 1] = 2.0; pts[:, 2] = -1.0
    pts[:, 3] = rng.random(len(pts), dtype=np.float32)
    ref = V.voxel_ref(pts, leaf)
    mn, mx = ref.box
    tight = V.floor_axis_counts(mn, mx, leaf)
    padded = (tight[0] + 32) * (tight[1] + 32) * (tight[2] + 8)
    assert not ref.unfiltered and padded > 4e9 and tight[0] * tight[1] * tight[2] < 4e9
    got, peak = _peak_filter(pts, leaf)
    print(f"{shape}: {peak / 1e9:.1f} GB of device memory held by the filter's handle")
    V.assert_matches_ref(got, ref, what=shape)
