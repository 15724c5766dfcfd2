"""The key-frame store beyond the front end (pcr_map_set_poses, _keyframe, _read_keyframe, _downsample_keyframes, _update_all, _view):
what Backend::optimHandler, LoopClosureManager::lcHandler, MapManager::saveKfs and test/vis_globalmap.cpp do to MapManager's key frames.

Device paths are compared byte for byte (the filter's order of additions depends on the sorted array alone); against
oracle.submap_assemble the bars are those of tests/test_submap_gpu.py: same point count, xyz atol 5e-4, intensity rtol 1e-5 / atol 1e-3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from simpleslam_amd import LoamRegister, SubMap, VgicpRegister, synth
from simpleslam_amd.pcr import PcrError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def keyframes():
    """The trajectory of tests/test_submap_gpu.py: 14 scans of 32 x 512 beams, each filtered at 0.4 -- a few thousand points per key frame,
    neighbouring key frames share voxels.  raw: the first six scans as they come from the sensor."""
    world, _ = synth.make_map(20_000, seed=91)
    kfs, raw = [], []
    for j in range(14):
        scan, T = synth.make_scan(world, j, seed=91, beams=32, azimuths=512)
        ds, _ = oracle.voxel_filter(scan, 0.4)
        kfs.append((ds, T))
        if j < 6:
            raw.append((scan, T))
    return world, kfs, raw


@pytest.fixture(scope="module")
def many_small():
    """50 key frames of 64 random points: more than the 48 descriptors a launch carries in its arguments"""
    rng = np.random.default_rng(50)
    out = []
    for j in range(50):
        pts = np.concatenate([rng.uniform(-5, 5, (64, 3)), rng.uniform(0, 100, (64, 1))], 1).astype(np.float32)
        T = synth.se3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-0.2, 0.2, 3)]))
        out.append((pts, T))
    return out


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _meets_oracle(got, ref):
    assert got.shape[0] == ref.shape[0]
    np.testing.assert_allclose(got[:, :3], ref[:, :3], rtol=0, atol=5e-4)
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=1e-3)


def _filled(kfs):
    sm = SubMap()
    for c, T in kfs:
        sm.addKeyFrame(c, T)
    return sm


def _turned(T, deg):
    """T with its heading turned by deg about the map's z"""
    a = np.deg2rad(deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    out = T.copy()
    out[:3, :3] = Rz @ T[:3, :3]
    return out


def _moved(T, d):
    out = T.copy()
    out[:3, 3] += d
    return out


def test_new_poses_take_effect_at_the_next_update_and_not_before(gpu, keyframes):
    world, kfs, _ = keyframes
    far = np.array([30.0, 0.0, 0.0])
    # key frame 5 starts 30 m away (the optimiser will bring it in), everything else on the trajectory
    start = [(c, _moved(T, far) if j == 5 else T) for j, (c, T) in enumerate(kfs)]
    sm = _filled(start)
    centre = kfs[6][1][:3, 3]
    n0 = sm.updateMap(centre, radius=8.0, grid_size=0.4)
    before, idx0, gen0 = sm.download(), sm.submapIdx(), sm.generation()
    assert 5 not in idx0 and 4 in idx0 and n0 == before.shape[0]
    # key frame 4 out of the radius, 5 into it, 6 .. 9 turned by a few degrees
    new = [_moved(kfs[4][1], far), kfs[5][1]] + [_turned(kfs[j][1], 0.5 * j - 1.0) for j in range(6, 10)]
    sm.setPoses(4, np.array(new))
    _same_bytes(sm.download(), before)
    np.testing.assert_array_equal(sm.submapIdx(), idx0)
    assert sm.generation() == gen0
    for j in range(6):
        np.testing.assert_array_equal(sm.keyFrame(4 + j)[1], new[j])
    # the next update: the oracle's selection and cloud under the new poses, and a store born with them, bit for bit
    poses = [T for _, T in kfs]
    poses[4:10] = new
    n = sm.updateMap(centre, radius=8.0, grid_size=0.4)
    ref, sel = oracle.submap_assemble([c for c, _ in kfs], poses, centre, 8.0, 0.4)
    np.testing.assert_array_equal(sm.submapIdx(), sel)
    assert 4 not in sel and 5 in sel
    got = sm.download()
    assert n == got.shape[0]
    _meets_oracle(got, ref)
    assert sm.generation() == (gen0[0], gen0[1] + 1)
    fresh = _filled([(c, P) for (c, _), P in zip(kfs, poses)])
    assert fresh.updateMap(centre, radius=8.0, grid_size=0.4) == n
    _same_bytes(got, fresh.download())
    # refused, and nothing changes: a range past the end, a view
    with pytest.raises(PcrError, match="exceeds"):
        sm.setPoses(10, np.array(new))
    with pytest.raises(PcrError, match="exceeds"):
        sm.setPoses(15, np.zeros((0, 4, 4)))
    sm.setPoses(14, np.zeros((0, 4, 4)))                                       # nothing at the very end: a no-op
    with pytest.raises(PcrError, match="view"):
        sm.view().setPoses(4, np.array(new))
    for j in range(14):
        np.testing.assert_array_equal(sm.keyFrame(j)[1], poses[j])


def test_radius_is_strict_and_in_double_for_poses_set_later(gpu):
    sm = SubMap()
    pts = np.array([[1.0, 0.0, 0.0, 5.0]], np.float32)
    for _ in range(4):
        T = np.eye(4); T[0, 3] = 100.0
        sm.addKeyFrame(pts, T)
    sm.updateMap(np.zeros(3), radius=8.0, grid_size=0.5)
    assert len(sm.submapIdx()) == 0
    P = np.tile(np.eye(4), (4, 1, 1))
    P[:, 0, 3] = (0.0, 3.0, 8.0, np.nextafter(8.0, 0.0))
    sm.setPoses(0, P)
    sm.updateMap(np.zeros(3), radius=8.0, grid_size=0.5)
    np.testing.assert_array_equal(sm.submapIdx(), [0, 1, 3])                   # the key frame at exactly 8 m is out (dist < radius)


def test_a_queued_assembly_finishes_under_the_poses_it_was_selected_with(gpu, keyframes):
    world, kfs, _ = keyframes
    whole, halves = _filled(kfs), _filled(kfs)
    centre = kfs[3][1][:3, 3]
    n = whole.updateMap(centre, radius=3.0, grid_size=0.4)
    halves.updateMapBegin(centre, radius=3.0, grid_size=0.4)
    halves.setPoses(0, np.array([_moved(_turned(T, 5.0), [1.0, 2.0, 0.0]) for _, T in kfs]))
    assert halves.wait() == n > 0
    np.testing.assert_array_equal(halves.submapIdx(), whole.submapIdx())
    _same_bytes(halves.download(), whole.download())


def test_a_views_window_leaves_the_parents_submap_alone(gpu, keyframes):
    world, kfs, _ = keyframes
    parent = _filled(kfs)
    scan, T_true = synth.make_scan(world, 10, seed=91, beams=32, azimuths=512)
    parent.updateMap(kfs[10][1][:3, 3], radius=3.0, grid_size=0.4)
    before, gen0 = parent.download(), parent.generation()
    reg = LoamRegister()
    ds = reg.voxelDownSample(scan, 0.4)
    p0 = synth.perturb(T_true, 3, trans=0.1, rot_deg=0.5)
    pa = p0.copy(); reg.scan2MapSubmap(ds, parent, pa)
    v = parent.view()
    n = v.loopFindNearKeyframes(3, 2, 0.4)
    np.testing.assert_array_equal(v.submapIdx(), [1, 2, 3, 4, 5])
    assert v.keyframes() == 14
    _same_bytes(parent.download(), before)
    assert parent.generation() == gen0
    assert v.generation()[0] != gen0[0]
    other = _filled(kfs)
    assert other.loopFindNearKeyframes(3, 2, 0.4) == n > 0
    _same_bytes(v.download(), other.download())
    # the front end's registrar has kept what it built from the parent's sub-map
    pb = p0.copy(); reg.scan2MapSubmap(ds, parent, pb)
    np.testing.assert_array_equal(pa, pb)
    assert reg.stats()["target_builds"] == 1
    # a view of a view is refused, and so is everything else that would change the store
    for call in (lambda: v.view(), lambda: v.addKeyFrame(*kfs[0]), lambda: v.clear(), lambda: v.downSampleKeyFrames(0, 0.4)):
        with pytest.raises(PcrError, match="view"):
            call()
    assert parent.keyframes() == 14


def test_loop_closure_from_the_stored_key_frame_against_a_view(gpu, keyframes):
    """tests/test_submap_gpu.py::test_loop_closure_flow with the odometry sub-map alive on the parent: the source is the stored key frame in
    HBM, the target a view's window.  Same pose, converged flag and fitness as with a host copy of the key frame and a separate store."""
    world, kfs, _ = keyframes
    key, rng = 6, 2
    scan, T_true = kfs[key]
    guess = synth.perturb(T_true, 7, trans=0.3, rot_deg=1.5)
    sep = _filled(kfs)
    sep.loopFindNearKeyframes(key, rng, grid_size=0.4)
    lc = VgicpRegister(); lc.initForLC()
    pose_ref = guess.copy()
    conv_ref = lc.scan2MapSubmap(scan, sep, pose_ref)
    fs_ref = lc.getFitnessScore()

    parent = _filled(kfs)
    parent.updateMap(kfs[12][1][:3, 3], radius=8.0, grid_size=0.4)
    odom, gen0 = parent.download(), parent.generation()
    v = parent.view()
    v.loopFindNearKeyframes(key, rng, grid_size=0.4)
    src = parent.keyFramePointer(key)
    assert src[1:] == (scan.shape[0], 16) and v.keyFramePointer(key) == src
    lc2 = VgicpRegister(); lc2.initForLC()
    pose = guess.copy()
    conv = lc2.scan2MapSubmap(src, v, pose)
    assert conv == conv_ref and conv
    np.testing.assert_array_equal(pose, pose_ref)
    assert lc2.getFitnessScore() == fs_ref
    _same_bytes(parent.download(), odom)
    assert parent.generation() == gen0


def test_the_store_moves_while_a_view_has_an_assembly_queued(gpu, many_small):
    parent = _filled(many_small[:3])
    v = parent.view()
    centre = np.zeros(3)
    n = v.updateMap(centre, radius=50.0, grid_size=0.4)
    expected = v.download()
    v.updateMapBegin(centre, radius=50.0, grid_size=0.4)
    # the store was sized for 16 key frames of 64 points and doubled: this one is far beyond twice that, the store moves
    rng = np.random.default_rng(5)
    big = np.concatenate([rng.uniform(-20, 20, (30_000, 3)), rng.uniform(0, 100, (30_000, 1))], 1).astype(np.float32)
    parent.addKeyFrame(big, np.eye(4))
    assert v.wait() == n > 0
    _same_bytes(v.download(), expected)
    np.testing.assert_array_equal(v.submapIdx(), [0, 1, 2])
    m = v.updateAll(0.4)
    np.testing.assert_array_equal(v.submapIdx(), [0, 1, 2, 3])
    assert m > n
    _same_bytes(parent.keyFrame(3)[0], big)


def test_clear_reaches_the_views_and_a_view_outlives_its_parent_harmlessly(gpu, keyframes):
    world, kfs, _ = keyframes
    parent = _filled(kfs[:5])
    v = parent.view()
    assert v.updateMap(kfs[2][1][:3, 3], radius=8.0, grid_size=0.4) > 0
    g = v.generation()
    v.updateMapBegin(kfs[1][1][:3, 3], radius=8.0, grid_size=0.4)                # (queued: waited for and dropped)
    parent.clear()
    assert v.pointer()[1] == 0 and len(v.submapIdx()) == 0 and v.keyframes() == 0 and v.wait() == 0
    assert v.generation()[0] == g[0] and v.generation()[1] > g[1] + 1
    parent.addKeyFrame(*kfs[0])
    assert v.updateAll(0.4) > 0
    # the parent goes first, at the C level (the Python objects would not allow it): the view refuses everything and can still be freed
    lib, pm, vm = parent._lib, parent._m, v._m
    parent._m = None
    lib.pcr_map_destroy(pm)
    n, s = C.c_size_t(7), C.c_size_t(7)
    i64, u64 = C.c_uint64(0), C.c_uint64(0)
    pos = (C.c_double * 3)(0, 0, 0)
    pose = (C.c_double * 16)()
    buf = (C.c_float * 64)()

    def refused(rc):
        assert rc != 0
        assert b"parent destroyed" in lib.pcr_map_last_error(vm)

    refused(lib.pcr_map_update(vm, pos, 8.0, 0.4, C.byref(n)))
    refused(lib.pcr_map_update_begin(vm, pos, 8.0, 0.4))
    refused(lib.pcr_map_wait(vm, C.byref(n)))
    refused(lib.pcr_map_update_window(vm, 0, 1, 0.4, C.byref(n)))
    refused(lib.pcr_map_update_all(vm, 0.4, C.byref(n)))
    refused(lib.pcr_map_keyframes(vm, C.byref(n)))
    refused(lib.pcr_map_generation(vm, C.byref(i64), C.byref(u64)))
    refused(lib.pcr_map_submap_indices(vm, None, 0, C.byref(n)))
    refused(lib.pcr_map_read_keyframe(vm, 0, buf, 16, C.byref(n), pose))
    refused(lib.pcr_map_add_keyframe(vm, buf, 4, 16, 0, pose))
    refused(lib.pcr_map_clear(vm))
    refused(lib.pcr_map_set_poses(vm, 0, 0, pose))
    refused(lib.pcr_map_downsample_keyframes(vm, 0, 0.4, C.byref(n)))
    refused(0 if lib.pcr_map_submap(vm, C.byref(n), C.byref(s)) else 1)
    assert n.value == 0
    refused(0 if lib.pcr_map_keyframe(vm, 0, C.byref(n), C.byref(s), pose) else 1)
    refused(0 if lib.pcr_map_view(vm) else 1)
    reg = LoamRegister()
    with pytest.raises(PcrError):
        reg.scan2MapSubmap(kfs[0][0], v, np.eye(4))
    v._m = None
    lib.pcr_map_destroy(vm)
    # and the usual order: a view freed before its parent is forgotten by it
    parent2 = _filled(kfs[:3])
    v2 = parent2.view()
    v2.updateAll(0.4)
    del v2
    parent2.addKeyFrame(*kfs[3])
    assert parent2.updateAll(0.4) > 0


def test_key_frames_filtered_in_place(gpu, keyframes):
    world, _, raw = keyframes
    reg = LoamRegister()
    sm = _filled(raw)
    sm.updateMap(raw[0][1][:3, 3], radius=8.0, grid_size=0.4)
    before, idx0, gen0 = sm.download(), sm.submapIdx(), sm.generation()
    filtered = [reg.voxelDownSample(scan, 0.4) for scan, _ in raw]
    after = sm.downSampleKeyFrames(2, 0.4)
    stored = [sm.keyFrame(j)[0] for j in range(6)]
    for j in range(6):
        _same_bytes(stored[j], raw[j][0] if j < 2 else filtered[j])
    assert all(0 < len(filtered[j]) < len(raw[j][0]) for j in range(6))
    assert after == sum(len(c) for c in stored)
    ptrs = [sm.keyFramePointer(j) for j in range(6)]
    for a, b in zip(ptrs, ptrs[1:]):
        assert b[0] == a[0] + a[1] * a[2]                                      # packed directly behind one another
    # what was assembled before stays as it is
    _same_bytes(sm.download(), before)
    np.testing.assert_array_equal(sm.submapIdx(), idx0)
    assert sm.generation() == gen0
    # and the store is now the store of those clouds
    fresh = _filled([(stored[j], raw[j][1]) for j in range(6)])
    centre = raw[3][1][:3, 3]
    n = fresh.updateMap(centre, radius=8.0, grid_size=0.4)
    assert sm.updateMap(centre, radius=8.0, grid_size=0.4) == n > 0
    _same_bytes(sm.download(), fresh.download())
    # the store goes on growing behind the compacted key frames
    sm.addKeyFrame(*raw[0]); fresh.addKeyFrame(*raw[0])
    assert sm.updateAll(0.4) == fresh.updateAll(0.4)
    _same_bytes(sm.download(), fresh.download())
    _same_bytes(sm.keyFrame(6)[0], raw[0][0])


def test_in_place_filter_edge_cases(gpu, many_small):
    import voxel_ref as V
    leaf, mn, mx = next(b for b in V.near_limit_boxes(900, seed=23) if V.pcl_too_fine(b[1], b[2], b[0]))
    too_fine = np.array([[*mn, 1.0], [*mx, 3.0]], np.float32)                   # PCL: "Leaf size is too small" -> the cloud as it is
    reg = LoamRegister()
    _same_bytes(reg.voxelDownSample(too_fine, leaf), too_fine)
    dense = many_small[1][0].copy()
    dense[:, :3] *= 0.01                                                       # 64 points within 0.1 m: at most 27 voxels at any leaf >= 0.05
    clouds = [many_small[0][0], np.zeros((0, 4), np.float32), too_fine, dense, np.zeros((0, 4), np.float32)]
    sm = _filled([(c, np.eye(4)) for c in clouds])
    want = [clouds[0]] + [reg.voxelDownSample(c, leaf) if len(c) else c for c in clouds[1:]]
    assert 0 < len(want[3]) < 64
    assert sm.downSampleKeyFrames(1, leaf) == sum(len(c) for c in want)
    for j in range(5):
        _same_bytes(sm.keyFrame(j)[0], want[j])
    assert sm.keyFramePointer(1) == (None, 0, 16) and sm.keyFramePointer(4) == (None, 0, 16)
    total = sum(len(c) for c in want)
    assert sm.downSampleKeyFrames(5, leaf) == total                             # first == count: nothing to do
    with pytest.raises(PcrError, match="exceeds"):
        sm.downSampleKeyFrames(6, leaf)
    for g in (0.0, -0.4, float("nan")):
        with pytest.raises(PcrError, match="positive"):
            sm.downSampleKeyFrames(0, g)
    for j in range(5):
        _same_bytes(sm.keyFrame(j)[0], want[j])
    # a store of nothing but empty key frames, and an empty store
    e = _filled([(np.zeros((0, 4), np.float32), np.eye(4))] * 2)
    assert e.downSampleKeyFrames(0, 0.4) == 0
    assert SubMap().downSampleKeyFrames(0, 0.4) == 0


def test_the_whole_map(gpu, keyframes, many_small):
    world, kfs, _ = keyframes
    for stock in (kfs, many_small):
        a, b = _filled(stock), _filled(stock)
        g0 = a.generation()
        n = a.updateAll(0.4)
        assert a.generation() == (g0[0], g0[1] + 1)
        np.testing.assert_array_equal(a.submapIdx(), np.arange(len(stock)))
        assert b.updateMap(stock[0][1][:3, 3], radius=1e9, grid_size=0.4) == n > 0
        got = a.download()
        _same_bytes(got, b.download())
        ref, sel = oracle.submap_assemble([c for c, _ in stock], [T for _, T in stock], np.zeros(3), 1e9, 0.4)
        assert len(sel) == len(stock) and n == got.shape[0]
        _meets_oracle(got, ref)
        v = a.view()                                                           # ... and on a view
        assert v.updateAll(0.4) == n
        _same_bytes(v.download(), got)
    empty = SubMap()
    assert empty.updateAll(0.4) == 0 and empty.pointer()[1] == 0 and len(empty.submapIdx()) == 0
    with pytest.raises(PcrError, match="positive"):
        empty.updateAll(0.0)


@pytest.mark.parametrize("floats", [8, 4])
def test_key_frames_read_back_as_stored(gpu, floats):
    rng = np.random.default_rng(floats)
    clouds = [rng.normal(0, 10, (n, floats)).astype(np.float32) for n in (257, 0, 1, 1000)]
    poses = [synth.se3_exp(rng.uniform(-1, 1, 6)) for _ in clouds]
    sm = _filled(zip(clouds, poses))
    v = sm.view()
    for who in (sm, v):
        for j, (c, T) in enumerate(zip(clouds, poses)):
            got, pose = who.keyFrame(j)
            _same_bytes(got, c)
            np.testing.assert_array_equal(pose, T)
            p, n, s = who.keyFramePointer(j)
            assert (n, s) == (len(c), floats * 4) and (p is None) == (len(c) == 0)
    new = synth.se3_exp(rng.uniform(-1, 1, 6))
    sm.setPoses(3, new)
    np.testing.assert_array_equal(v.keyFrame(3)[1], new)
    np.testing.assert_array_equal(sm.keyFrame(2)[1], poses[2])
    with pytest.raises(PcrError, match="out of range"):
        sm.keyFrame(4)
    with pytest.raises(PcrError, match="out of range"):
        v.keyFramePointer(4)
    # too little room: an error, the size reported, nothing written
    lib = sm._lib
    out = np.full((999, floats), 7.0, np.float32)
    pose = np.full(16, 7.0)
    n = C.c_size_t(0)
    dp = C.POINTER(C.c_double)
    assert lib.pcr_map_read_keyframe(sm._m, 3, out.ctypes.data_as(C.c_void_p), 999, C.byref(n), pose.ctypes.data_as(dp)) != 0
    assert n.value == 1000 and b"1000" in lib.pcr_map_last_error(sm._m)
    assert (out == 7.0).all() and (pose == 7.0).all()
    assert lib.pcr_map_read_keyframe(sm._m, 4, out.ctypes.data_as(C.c_void_p), 999, C.byref(n), pose.ctypes.data_as(dp)) != 0
    assert lib.pcr_map_keyframe(sm._m, 4, C.byref(n), None, None) is None and b"out of range" in lib.pcr_map_last_error(sm._m)
    assert lib.pcr_map_read_keyframe(sm._m, 1, None, 0, C.byref(n), pose.ctypes.data_as(dp)) == 0 and n.value == 0      # an empty key frame: rc 0
    np.testing.assert_array_equal(pose, poses[1].T.reshape(16))


def test_map_check_program(gpu):
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "map_check")
    assert os.path.exists(exe), "map_check not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "map_check ok"
