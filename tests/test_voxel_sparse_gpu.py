"""pcp::VoxelDownSampleV3 and pcp::VoxelDownSampleV2 on the device (pcr_voxel_filter_sparse, pcr_voxel_sparse_order, pcr_map_update_all_sparse)
against the numpy and dict restatement in tests/voxel_sparse_ref.py.

V3: the same rows as the restatement, every averaged channel within one float32 ulp of the float64 mean (the standing criterion of
tests/test_voxel_edges_gpu.py: a point in the wrong voxel moves a centroid by far more).  V2: bit for bit -- at most max_voxel_pts float
additions in a defined order.  The sort: keys and rows exactly numpy's stable argsort of the restated keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import submap_ref as R
import voxel_ref as V
import voxel_sparse_ref as S
from simpleslam_amd import LoamRegister, NdtRegister, SubMap
from simpleslam_amd.pcr import PcrError, VoxelSparseParams
from tests import loc_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSCHK = os.path.join(ROOT, "simpleslam_amd", "lib", "voxel_sparse_check")


@pytest.fixture(scope="module")
def reg(gpu):
    return LoamRegister()


def _both(reg, pts, leaf, what, max_pts=20, min_pts=0):
    """both kinds against the restatement -> (V3 output, V2 output)"""
    a = reg.voxelDownSampleV3(pts, leaf)
    S.assert_v3(a, S.sparse_ref(pts, leaf, S.V3), what=f"V3 {what}")
    b = reg.voxelDownSampleV2(pts, leaf, max_pts, min_pts)
    S.assert_v2(b, S.sparse_ref(pts, leaf, S.V2, max_pts, min_pts), what=f"V2 {what}")
    return a, b


# ---------------------------------------------------------------------------
# beyond pcl::VoxelGrid's range
# ---------------------------------------------------------------------------
def test_beyond_pcls_range_63_key_bits(reg):
    """512 clusters of 8 points over a box of 2^21 leaves per axis (63 key bits, 9.2e18 voxels): pcl::VoxelGrid -- and pcr_voxel_filter -- return the
    input unfiltered; the sparse filters return the restatement's rows.  No table over that box exists: that it runs at all is the proof."""
    rng = np.random.default_rng(11)
    leaf, side = 1.0, 2 ** 21
    centres = rng.integers(8, side - 8, (512, 3)).astype(np.float64)
    pts = np.zeros((4096 + 2, 4), np.float32)
    pts[:4096, :3] = (np.repeat(centres, 8, axis=0) + rng.integers(-6, 7, (4096, 3)) * 0.25).astype(np.float32)      # (multiples of 0.25: floats up to 2^21 hold them)
    pts[4096, :3] = 0.0
    pts[4097, :3] = side - 1
    pts[:, 3] = rng.random(len(pts), dtype=np.float32) * 100
    pts = pts[rng.permutation(len(pts))]
    ref = S.sparse_ref(pts, leaf, S.V3)
    assert ref.bits == (21, 21, 21) and V.voxel_ref(pts, leaf).unfiltered
    np.testing.assert_array_equal(reg.voxelDownSample(pts, leaf), pts)
    a, b = _both(reg, pts, leaf, "2^21 leaves per axis")
    assert 512 < len(a) < 4098 and len(b) == len(a)


# ---------------------------------------------------------------------------
# agreement with the PCL filter where both filter
# ---------------------------------------------------------------------------
def _agree(reg, pts, leaf, what):
    pcl = V.voxel_ref(pts, leaf)
    assert not pcl.unfiltered
    got_pcl = reg.voxelDownSample(pts, leaf)
    V.assert_matches_ref(got_pcl, pcl, what=f"pcr_voxel_filter {what}")
    a, _ = _both(reg, pts, leaf, what)
    # the same count, the same voxel per row, the same order: both are within an ulp of the float64 mean of the SAME members, row by row
    ref = S.sparse_ref(pts, leaf, S.V3)
    assert len(a) == len(got_pcl) == len(pcl)
    assert all(ref.members[i] == pcl.members(i).tolist() for i in range(len(pcl)))
    assert S.ulp_distance(a, got_pcl).max() <= 2


def test_agrees_with_the_pcl_filter_on_a_scan(reg, world_small):
    _agree(reg, world_small["scan"], 0.4, "scan")


@pytest.mark.parametrize("leaf,sign", [(0.05, 1.0), (0.1, -1.0), (0.3, 1.0), (0.5, -1.0)])
def test_agrees_with_the_pcl_filter_on_voxel_faces(reg, leaf, sign):
    pts, _ = V.face_cloud(leaf, sign, n=6000, seed=int(leaf * 1000), only_disagreeing=leaf != 0.5)
    _agree(reg, pts, leaf, f"faces {leaf} {sign}")


@pytest.mark.parametrize("leaf,log2_ratio,sign", [(0.05, 23.1, 1.0), (0.1, 23.5, -1.0), (0.3, 24.9, 1.0), (0.25, 24.2, -1.0)])
def test_agrees_with_the_pcl_filter_far_from_the_origin(reg, leaf, log2_ratio, sign):
    _agree(reg, V.far_cloud(leaf, log2_ratio, sign, n=6000, seed=int(log2_ratio * 10)), leaf, f"far {leaf} 2^{log2_ratio}")


# ---------------------------------------------------------------------------
# the sort
# ---------------------------------------------------------------------------
def _check_order(reg, pts, leaf=1.0, kind=S.V3):
    out = reg.voxelDownSampleV3(pts, leaf) if kind == S.V3 else reg.voxelDownSampleV2(pts, leaf)
    keys, rows = reg.sparseOrder()
    want_k, want_r = S.sorted_pairs(pts, leaf, kind)
    np.testing.assert_array_equal(keys, want_k)
    np.testing.assert_array_equal(rows, want_r)
    assert len(out) == len(np.unique(want_k))
    return keys


def _triples(n, bits, seed, distinct=600):
    """n rows on integer triples (leaf 1) whose packed key takes bits = (bx, by, bz): the two corners of the box, and rows drawn with repeats
    from `distinct` random triples inside it"""
    rng = np.random.default_rng(seed)
    hi = np.array([(1 << b) - 1 for b in bits], np.int64)
    pool = np.stack([rng.integers(0, h + 1, distinct) for h in hi], axis=1)
    t = pool[rng.integers(0, distinct, n)]
    t[rng.integers(0, n)] = 0
    t[rng.integers(0, n)] = hi
    t[0], t[-1] = hi, 0
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = t - hi // 2                      # (around the origin: floats hold every integer below 2^24)
    pts[:, 3] = np.arange(n)
    return pts


# wave 64, block 256, the scans' 1024 threads, the digit passes' tile of 2048, and a second and fifth tile
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193])
def test_sort_at_block_and_tile_edges(reg, n):
    for kind in (S.V3, S.V2):
        _check_order(reg, _triples(n, (4, 3, 3), seed=n, distinct=min(n, 300)), kind=kind)


def test_sort_all_rows_in_one_voxel(reg):
    rng = np.random.default_rng(2)
    pts = np.zeros((100_000, 4), np.float32)
    pts[:, :3] = 5.0 + 0.9 * rng.random((100_000, 3), dtype=np.float32)
    pts[:, 3] = rng.random(100_000, dtype=np.float32)
    keys = _check_order(reg, pts)
    assert not keys.any()
    S.assert_v3(reg.voxelDownSampleV3(pts, 1.0), S.sparse_ref(pts, 1.0, S.V3), what="100 000 rows in one voxel")
    S.assert_v2(reg.voxelDownSampleV2(pts, 1.0), S.sparse_ref(pts, 1.0, S.V2), what="100 000 rows in one voxel")


def test_sort_all_rows_in_distinct_voxels_and_more_blocks_than_scan_threads(reg):
    """70 x 70 x 54 = 264 600 voxels with a row each, shuffled: more than 1024 blocks of 256 sorted rows, so the scan of the per-block counts gives
    a thread more than one entry"""
    g = np.stack(np.meshgrid(np.arange(70), np.arange(70), np.arange(54), indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.zeros((len(g), 4), np.float32)
    pts[:, :3] = g[np.random.default_rng(4).permutation(len(g))] + 0.5
    keys = _check_order(reg, pts)
    assert len(np.unique(keys)) == len(pts) > 256 * 1024
    out = reg.voxelDownSampleV3(pts, 1.0)
    np.testing.assert_array_equal(out[:, :3], g[np.lexsort((g[:, 0], g[:, 1], g[:, 2]))] + 0.5)


@pytest.mark.parametrize("bits", [(1, 0, 0), (3, 3, 2), (3, 3, 3), (6, 5, 5), (6, 6, 5), (14, 13, 13), (22, 21, 21)])
def test_sort_key_widths_at_digit_boundaries(reg, bits):
    """1, 8, 9, 16, 17, 40 and 64 key bits: one digit pass to eight"""
    pts = _triples(3000, bits, seed=sum(bits))
    keys = _check_order(reg, pts)
    assert int(keys.max()) == (1 << sum(bits)) - 1 and int(keys.min()) == 0
    _check_order(reg, pts, kind=S.V2)


def _axis(b):
    """(lo, hi) of an axis whose extent takes b key bits, both exact floats inside the int range"""
    return (0.0, 0.0) if b == 0 else ((0.0, float(1 << (b - 1))) if b <= 31 else (-2.0 ** 31, 2.0 ** 30))


@pytest.mark.parametrize("width,low_bits,high_bits", [(9, (1, 4, 4), (3, 3, 3)), (17, (1, 8, 8), (6, 6, 5)), (64, (1, 31, 32), (22, 21, 21))])
def test_sort_keys_that_differ_in_one_bit_only(reg, width, low_bits, high_bits):
    """5000 rows in two voxels whose keys differ only in the lowest used bit (x = 0 / 1 under the largest y and z), and only in the highest
    (z at either end under the smallest x and y); one more row pins the extents of the other axes"""
    rng = np.random.default_rng(width)
    n = 5000
    for bits, which in ((low_bits, "low"), (high_bits, "high")):
        (x0, x1), (y0, y1), (z0, z1) = (_axis(b) for b in bits)
        pts = np.zeros((n + 1, 4), np.float32)
        pick = rng.integers(0, 2, n)
        if which == "low":
            pts[:n, :3] = np.stack([np.where(pick, x1, x0), np.full(n, y1), np.full(n, z1)], axis=1)
            pts[n, :3] = [x0, y0, z0]
        else:
            pts[:n, :3] = np.stack([np.full(n, x0), np.full(n, y0), np.where(pick, z1, z0)], axis=1)
            pts[n, :3] = [x1, y1, z0]
        pts[:, 3] = np.arange(n + 1)
        pts = pts[rng.permutation(n + 1)]
        keys = _check_order(reg, pts)
        k_all = S.pack(S.lattice(pts, 1.0, S.V3)[1], S.V3)
        assert sum(k_all[2]) == width
        two = np.unique(k_all[3][pts[:, 3] < n])
        assert len(two) == 2 and int(two[0]) ^ int(two[1]) == (1 if which == "low" else 1 << (width - 1))
        assert len(np.unique(keys)) == 3


def test_65_key_bits_are_refused_with_the_extents(reg):
    pts = np.zeros((3, 4), np.float32)
    pts[1, :3] = [2 ** 22 - 1, 2 ** 22 - 1, 2 ** 21 - 1]
    pts[2, :3] = [5, 5, 5]
    for f in (reg.voxelDownSampleV3, reg.voxelDownSampleV2):
        with pytest.raises(PcrError) as e:
            f(pts, 1.0)
        assert "65 bits" in str(e.value) and "4194304 x 4194304 x 2097152" in str(e.value)
        with pytest.raises(PcrError):
            reg.sparseOrder()
    pts[1, 1] = 2 ** 21 - 1                 # 64 bits: served
    _check_order(reg, pts)


def test_int_range_is_refused(reg):
    pts = np.zeros((3, 4), np.float32)
    pts[1, 0] = 3.0e9
    for f, name in ((reg.voxelDownSampleV3, "floor(p * inv)"), (reg.voxelDownSampleV2, "p / gs")):
        with pytest.raises(PcrError) as e:
            f(pts, 1.0)
        assert name in str(e.value) and "int range" in str(e.value)
    pts[1, 0] = -2.0 ** 31                  # INT_MIN is an int
    _both(reg, pts, 1.0, "INT_MIN")


# ---------------------------------------------------------------------------
# V2's dependence on the order of the rows
# ---------------------------------------------------------------------------
def _v2_cloud(seed, cap=20):
    """voxels (leaf 1, around and below zero) of cap - 1, cap and cap + 1 rows whose LAST row is an outlier at the far corner of its voxel"""
    rng = np.random.default_rng(seed)
    chunks = []
    for k, m in enumerate([cap - 1, cap, cap + 1, cap + 7, 1, 2]):
        base = np.array([-3.0 * k - 1.0, 2.0 * (k % 2) - 3.0, -1.0 - k], np.float32)      # (negative coordinates: truncation toward zero)
        c = np.zeros((m, 4), np.float32)
        c[:, :3] = base - 0.1 * rng.random((m, 3), dtype=np.float32)
        c[-1, :3] = base - 0.95
        c[:, 3] = 100 * k + np.arange(m)
        chunks.append(c)
    return chunks


def test_v2_keeps_the_rows_of_lowest_index(reg):
    chunks = _v2_cloud(5)
    pts = np.concatenate(chunks)
    inter = pts[np.random.default_rng(6).permutation(len(pts))]           # another order of the same rows
    for name, cloud in (("by voxel", pts), ("reversed", pts[::-1].copy()), ("shuffled", inter)):
        ref = S.sparse_ref(cloud, 1.0, S.V2)
        assert len(ref.out) == 6 and sorted(len(m) for m in ref.members) == [1, 2, 19, 20, 20, 20]
        S.assert_v2(reg.voxelDownSampleV2(cloud, 1.0), ref, what=name)
    a, b = S.sparse_ref(pts, 1.0, S.V2), S.sparse_ref(pts[::-1].copy(), 1.0, S.V2)
    assert not np.array_equal(a.out, b.out)                              # the surplus row is an outlier: which rows are kept shows in the mean
    for cap in (1, 19, 21, 27, 28):
        S.assert_v2(reg.voxelDownSampleV2(inter, 1.0, cap), S.sparse_ref(inter, 1.0, S.V2, cap), what=f"cap {cap}")


@pytest.mark.parametrize("min_pts", [0, 1, 2, 18, 19, 20, 21])
def test_v2_min_voxel_pts_is_strict(reg, min_pts):
    pts = np.concatenate(_v2_cloud(8))[np.random.default_rng(9).permutation(90)]
    ref = S.sparse_ref(pts, 1.0, S.V2, 20, min_pts)
    assert len(ref.out) == {0: 6, 1: 5, 2: 4, 18: 4, 19: 3, 20: 0, 21: 0}[min_pts]
    S.assert_v2(reg.voxelDownSampleV2(pts, 1.0, 20, min_pts), ref, what=f"min_voxel_pts {min_pts}")


def test_v2_double_width_voxels_about_zero(reg):
    rng = np.random.default_rng(10)
    pts = np.zeros((4000, 4), np.float32)
    pts[:, :3] = rng.uniform(-1.2, 1.2, (4000, 3))
    pts[:, 3] = np.arange(4000)
    ref = S.sparse_ref(pts, 0.4, S.V2)
    assert ref.extents == (5, 5, 5) and S.sparse_ref(pts, 0.4, S.V3).extents == (6, 6, 6)
    _both(reg, pts, 0.4, "about zero")


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nan_axis0", "+inf_axis1", "-inf_axis2", "duplicates", "voxel_sizes"])
def test_awkward_content(reg, name):
    pts, leaf = V.awkward_clouds()[name]
    _both(reg, pts, leaf, name)
    if "axis" in name:
        assert len(reg.sparseOrder()[1]) == len(pts) - 97


def test_empty_and_all_non_finite(reg):
    for f in (reg.voxelDownSampleV3, reg.voxelDownSampleV2):
        assert f(np.zeros((0, 4), np.float32), 0.4).shape == (0, 4)
        assert len(reg.sparseOrder()[0]) == 0
        bad = np.full((300, 4), np.nan, np.float32)
        bad[::2] = [1.0, np.inf, 0.0, 1.0]
        assert f(bad, 0.4).shape == (0, 4)
        assert len(reg.sparseOrder()[0]) == 0


def _raw(reg, pts, leaf, prm, capacity, in_dev, out_dev):
    """pcr_voxel_filter_sparse as the C ABI has it -> (rc, n_out, output as a host array of `capacity` rows)"""
    import torch
    n, sf = pts.shape
    src = torch.from_numpy(pts).cuda() if in_dev else pts
    p = C.c_void_p(src.data_ptr()) if in_dev else src.ctypes.data_as(C.c_void_p)
    out = torch.zeros((max(capacity, 1), sf), dtype=torch.float32, device="cuda") if out_dev else np.zeros((max(capacity, 1), sf), np.float32)
    o = C.c_void_p(out.data_ptr()) if out_dev else out.ctypes.data_as(C.c_void_p)
    cnt = C.c_size_t(0)
    rc = reg._lib.pcr_voxel_filter_sparse(reg._h, p, n, sf * 4, int(in_dev), float(leaf), C.byref(prm) if prm is not None else None, o, capacity, int(out_dev),
                                          C.byref(cnt))
    return rc, cnt.value, (out.cpu().numpy() if out_dev else out)


def test_capacity_too_small_returns_the_count(reg, world_small):
    pts = world_small["scan"]
    for prm in (VoxelSparseParams(3, 20, 0), VoxelSparseParams(2, 20, 0)):
        ref = S.sparse_ref(pts, 0.4, prm.kind)
        rc, cnt, _ = _raw(reg, pts, 0.4, prm, 10, False, False)
        assert rc != 0 and cnt == len(ref.out) and "capacity" in reg._lib.pcr_last_error(reg._h).decode()
        rc, cnt, out = _raw(reg, pts, 0.4, prm, cnt, True, True)             # the retry, with exactly that room
        assert rc == 0 and cnt == len(ref.out)
        (S.assert_v3 if prm.kind == 3 else S.assert_v2)(out[:cnt], ref, what="retry")


@pytest.mark.parametrize("stride", [3, 4, 5, 6, 7, 8])
def test_strides_host_and_device_in_and_out(reg, stride):
    src, _ = V.face_cloud(0.1, -1.0, n=3000, seed=stride)
    pts = np.random.default_rng(stride).random((src.shape[0], stride), dtype=np.float32) * 7
    pts[:, :3] = src[:, :3]
    for prm in (None, VoxelSparseParams(2, 3, 0)):                          # NULL parameters: V3
        kind = 3 if prm is None else 2
        ref = S.sparse_ref(pts, 0.1, kind, 3, 0)
        outs = []
        for in_dev in (False, True):
            for out_dev in (False, True):
                rc, cnt, out = _raw(reg, pts, 0.1, prm, len(pts), in_dev, out_dev)
                assert rc == 0, reg._lib.pcr_last_error(reg._h).decode()
                (S.assert_v3 if kind == 3 else S.assert_v2)(out[:cnt], ref, what=f"stride {stride} in {in_dev} out {out_dev}")
                outs.append(out[:cnt].tobytes())
        assert len(set(outs)) == 1                                           # the same bytes whichever way, and call after call


def test_the_same_call_twice_is_byte_identical(reg, world_small):
    """on one handle and on a fresh one: the output and what was sorted, byte for byte"""
    import torch
    d = torch.from_numpy(world_small["map"]).cuda()
    for name in ("voxelDownSampleV3", "voxelDownSampleV2"):
        runs = []
        for r in (reg, reg, LoamRegister()):
            out = getattr(r, name)(d, 0.4).cpu().numpy().tobytes()
            runs.append((out,) + tuple(x.tobytes() for x in r.sparseOrder()))
        assert runs[0] == runs[1] == runs[2] and len(runs[0][0]) > 0


def test_any_method_serves_it(gpu, world_small):
    pts = world_small["scan"][:3000]
    S.assert_v3(NdtRegister().voxelDownSampleV3(pts, 0.4), S.sparse_ref(pts, 0.4, S.V3), what="ndt handle")


def test_refused_parameters_are_named(reg):
    pts = np.ones((4, 4), np.float32)
    for prm, leaf, word in ((VoxelSparseParams(3, 20, 0), 0.0, "leaf"), (VoxelSparseParams(3, 20, 0), -1.0, "leaf"), (VoxelSparseParams(3, 20, 0), 1e-60, "leaf"),
                            (VoxelSparseParams(2, 0, 0), 0.4, "max_voxel_pts"), (VoxelSparseParams(2, 20, -1), 0.4, "min_voxel_pts"),
                            (VoxelSparseParams(4, 20, 0), 0.4, "kind")):
        rc, cnt, _ = _raw(reg, pts, leaf, prm, 4, False, False)
        assert rc != 0 and cnt == 0 and word in reg._lib.pcr_last_error(reg._h).decode()
    rc, _, _ = _raw(reg, pts, 0.4, VoxelSparseParams(3, 0, -5), 4, False, False)      # V2's fields are not read for V3
    assert rc == 0


# ---------------------------------------------------------------------------
# the whole map
# ---------------------------------------------------------------------------
def _keyframes(spread, seed=21, n_kf=5, n=3000):
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for j in range(n_kf):
        c = np.zeros((n + j, 4), np.float32)
        c[:, :3] = rng.uniform(-6, 6, (n + j, 3))
        c[:, 3] = rng.random(n + j, dtype=np.float32) * 100
        clouds.append(c)
        poses.append(R.pose(rng.uniform(-1, 1, 3), rng.uniform(-spread, spread, 3)))
    return clouds, poses


def test_update_all_sparse_is_the_sparse_filter_of_the_concatenation(reg):
    clouds, poses = _keyframes(3.0)
    cat = np.concatenate([R.transform(c, T) for c, T in zip(clouds, poses)])
    want = reg.voxelDownSampleV3(cat, 0.4)
    S.assert_v3(want, S.sparse_ref(cat, 0.4, S.V3), what="concatenation")
    sm = SubMap()
    for c, T in zip(clouds, poses):
        sm.addKeyFrame(c, T)
    for m in (sm, sm.view()):
        g0 = m.generation()[1]
        assert m.updateAllSparse(0.4) == len(want)
        assert m.generation()[1] == g0 + 1 and m.submapIdx().tolist() == list(range(len(clouds)))
        assert m.download().tobytes() == want.tobytes()
        m.updateMapBegin(np.zeros(3), radius=100.0, grid_size=0.4)          # a queued assembly is collected first
        assert m.updateAllSparse(0.4) == len(want) and m.download().tobytes() == want.tobytes()
        assert m.generation()[1] == g0 + 3
    assert sm.updateAll(0.4) == len(want)                                    # (PCL's filter serves this map too: the same voxels)


def test_update_all_sparse_filters_a_map_too_wide_for_pcl(reg):
    """key frames 3e5 m apart at a 0.2 m leaf: updateAll returns the concatenation unfiltered, updateAllSparse the filtered map"""
    clouds, poses = _keyframes(3.0e5, seed=22, n_kf=4, n=1500)
    cat = np.concatenate([R.transform(c, T) for c, T in zip(clouds, poses)])
    assert V.voxel_ref(cat, 0.2).unfiltered
    ref = S.sparse_ref(cat, 0.2, S.V3)
    sm = SubMap()
    for c, T in zip(clouds, poses):
        sm.addKeyFrame(c, T)
    assert sm.updateAll(0.2) == len(cat)
    np.testing.assert_array_equal(sm.download(), cat)
    assert sm.updateAllSparse(0.2) == len(ref.out) < len(cat)
    S.assert_v3(sm.download(), ref, what="wide map")


# ---------------------------------------------------------------------------
# the C++ mirror
# ---------------------------------------------------------------------------
def _fnv(rows):
    h = 1469598103934665603
    for b in np.ascontiguousarray(rows[:, :5], np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_mirror_matches_python(reg, tmp_path, world_small):
    pts = world_small["scan"][:6000]
    loc_inputs.write_pcd(tmp_path / "c.pcd", pts, "binary")
    r = subprocess.run([VSCHK, str(tmp_path / "c.pcd"), "0.4", "5", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict((ln.split()[0], ln.split()[1:]) for ln in r.stdout.splitlines())
    p8 = R.widen(pts, 8)
    a, b = reg.voxelDownSampleV3(p8, 0.4), reg.voxelDownSampleV2(p8, 0.4, 5, 1)
    assert lines["input"] == [str(len(pts))]
    assert lines["v3"] == [str(len(a)), f"{_fnv(a):016x}"] and lines["v3_in_place"] == lines["v3"]
    assert lines["v2"] == [str(len(b)), f"{_fnv(b):016x}"]
