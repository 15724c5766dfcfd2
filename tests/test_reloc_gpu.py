"""Relocalisation from a coarse pose on the device: the batched gated fitness score (pcr_fitness_batch, reloc.hip) against brute force
(tests/fitness_ref.py) and against the single-pose pcr_fitness_gated on every kind of index, and pcr_relocalize end to end: from a click
that a plain align does not recover from, to the true pose."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import fitness_ref as fr
import oracle
from simpleslam_amd import LoamRegister, NdtRegister, VgicpRegister, reloc_hypotheses, synth
from simpleslam_amd.pcr import PcrError
from test_fitness_gpu import HANDLES
from test_reloc_host import restated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = fr.DBL_MAX


def _ref_d2(src, dst, pose):
    """per-point float squared 1-NN distance of the transformed source; inf where a coordinate is not finite"""
    q = fr.transform_f32(src, pose)
    ok = np.isfinite(q).all(axis=1)
    d2 = np.full(len(q), np.inf, np.float32)
    if ok.any():
        _, d = oracle.knn_f32(dst, q[ok], 1)
        d2[ok] = d[:, 0]
    return d2


def _subset(n, score_points):
    if score_points == 0 or score_points >= n:
        return np.arange(n)
    return (np.arange(score_points, dtype=np.int64) * n) // score_points


def _assert_batch(got, src, dst, poses, max_sq, score_points=0, what=""):
    scores, n_in = got
    idx = _subset(len(src), score_points)
    for k, T in enumerate(poses):
        want_s, want_n = fr.gated_from_sq(_ref_d2(src[idx], dst, T), max_sq)
        assert n_in[k] == want_n, (what, k, n_in[k], want_n)
        if want_n == 0:
            assert scores[k] == -1.0, (what, k, scores[k])
        else:
            np.testing.assert_allclose(scores[k], want_s, rtol=fr.sum_order_rtol(want_n), atol=0, err_msg=f"{what} pose {k}")


def _planar(T, dx, dy, yaw_deg):
    """T moved in the map's plane: Rz(yaw) about the sensor, then (dx, dy, 0)"""
    a = math.radians(yaw_deg)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    out = T.copy()
    out[:3, :3] = Rz @ T[:3, :3]
    out[:3, 3] += [dx, dy, 0.0]
    return out


@pytest.fixture(scope="module")
def scored_world():
    world, m = synth.make_map(40_000, seed=31)
    scan, T = synth.make_scan(world, 0, seed=31, beams=16, azimuths=512)
    src = scan.copy()
    src[::97, 0] = np.nan; src[5::131, 1] = np.inf; src[11::173, 2] = -np.inf      # rows that are not counted
    poses = [synth.perturb(T, 100 + k, trans=0.1 + 0.05 * k, rot_deg=0.5 + 0.3 * k) for k in range(40)]
    poses += [_planar(T, dx, dy, yaw) for dx, dy, yaw in ((1.0, -0.5, 10.0), (-2.0, 1.5, -25.0), (0.5, 0.5, 90.0), (3.0, 0.0, 0.0))]
    poses += [_planar(T, 500.0, 0.0, 0.0), _planar(T, 0.0, -800.0, 30.0), _planar(T, 2e4, 2e4, 0.0)]      # off the map
    poses += [T, np.eye(4), synth.perturb(T, 7, trans=1.0, rot_deg=5.0)]
    return dict(map=m, scan=scan, src=src, truth=T, poses=np.array(poses))


@pytest.mark.parametrize("name", list(HANDLES))
def test_batch_against_brute_force(gpu, scored_world, name):
    """~50 poses (some off the map), a source with NaN / inf rows: n_in exact, score within another summation order's bound; the same on
    a score_points subset against brute force on the restated subset"""
    cls, kw, _ = HANDLES[name]
    w = scored_world
    reg = cls(**kw)
    reg.setTarget(w["map"])
    for max_sq in (1.0, 0.05, DBL_MAX):
        _assert_batch(reg.fitnessBatch(w["src"], w["poses"], max_sq), w["src"], w["map"], w["poses"], max_sq, 0, (name, max_sq))
    for sp in (1000, 4097, 1):
        _assert_batch(reg.fitnessBatch(w["src"], w["poses"], 1.0, sp), w["src"], w["map"], w["poses"], 1.0, sp, (name, "subset", sp))
    s, n = reg.fitnessBatch(w["src"], w["poses"][:3], 1.0, len(w["src"]) + 5)     # >= n_src: every point
    s0, n0 = reg.fitnessBatch(w["src"], w["poses"][:3], 1.0, 0)
    assert (s == s0).all() and (n == n0).all()


@pytest.mark.parametrize("name", ["loam", "ndt1", "vgicp05"])
def test_one_pose_is_the_single_pose_call_bit_for_bit(gpu, scored_world, name):
    """K = 1 (and every pose of a batch) equals pcr_fitness_gated for that pose: the same count, the same double, for the whole source
    and for a subset (gathered on the host for the single-pose call); device and host sources alike"""
    import torch
    cls, kw, _ = HANDLES[name]
    w = scored_world
    reg = cls(**kw)
    reg.setTarget(w["map"])
    src, poses = w["src"], w["poses"]
    d_src = torch.from_numpy(src).cuda()
    for sp in (0, 3000):
        sub = np.ascontiguousarray(src[_subset(len(src), sp)])
        batch = reg.fitnessBatch(d_src, poses, 1.0, sp)
        for k in range(0, len(poses), 5):
            one = reg.fitnessBatch(src, poses[k:k + 1], 1.0, sp)
            single = reg.fitnessGated(sub, poses[k], 1.0)
            assert (one[0][0], int(one[1][0])) == single, (name, sp, k, one, single)
            assert (batch[0][k], int(batch[1][k])) == single, (name, sp, k)


def test_gate_is_exact_on_lattice_ties(gpu):
    """a 1 m lattice target and a source half a cell off it (two nearest points at once): every source point's distance is exactly 0.25
    under every pose that moves by whole cells or turns by 90 degrees; max_sq = 0.25 counts them all, one float below counts none"""
    g = np.stack(np.meshgrid(np.arange(-6, 7), np.arange(-6, 7), np.arange(0, 4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    tgt = np.zeros((len(g), 4), np.float32); tgt[:, :3] = g
    inner = g[(np.abs(g[:, 0]) <= 2) & (np.abs(g[:, 1]) <= 2)]
    src = np.zeros((len(inner), 4), np.float32); src[:, :3] = inner + np.float32([0.5, 0.0, 0.0])
    poses = []
    for dx in (-2, -1, 0, 1, 2):
        for dy in (-1, 0, 1):
            T = np.eye(4); T[:3, 3] = [dx, dy, 0]
            poses.append(T)
    R90 = np.eye(4); R90[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    poses.append(R90)
    D = 0.25
    assert (fr.nearest_sq(fr.transform_f32(src, poses[0]), tgt)[0] == np.float32(D)).all()
    for name in ("loam", "ndt1", "vgicp1"):
        cls, kw, _ = HANDLES[name]
        reg = cls(**kw)
        reg.setTarget(tgt)
        for gate in (D, float(np.nextafter(np.float32(D), np.float32(0))), float(np.nextafter(D, 0.0)), float(np.nextafter(D, 1.0))):
            s, n = reg.fitnessBatch(src, poses, gate)
            _assert_batch((s, n), src, tgt, poses, gate, 0, (name, gate))
            if gate < D:
                assert (n == 0).all() and (s == -1.0).all(), (name, gate, n)
            else:
                assert (n == len(src)).all() and (s == D).all(), (name, gate, n, s)


@pytest.fixture(scope="module")
def cut_world():
    """the map plus a thinned copy 30 km away and a stray point beyond the bulk box: the target index is cut to the bulk"""
    world, m = synth.make_map(60_000, seed=21)
    scan, T = synth.make_scan(world, 0, seed=21, beams=32, azimuths=512)
    off = np.array([30000.0, 20000.0, 8000.0], np.float32)
    far = m[::200].copy(); far[:, :3] += off
    stray = np.zeros((1, 4), np.float32); stray[0, :3] = m[:, :3].min(axis=0) - np.float32([60.0, 0.0, 0.0])
    both = np.ascontiguousarray(np.vstack([m, far, stray]))
    there = T.copy(); there[:3, 3] += off
    poses = [synth.perturb(T, 200 + k, trans=0.3 * k, rot_deg=2.0 * k) for k in range(8)]
    poses += [there, _planar(there, 3.0, -2.0, 15.0), _planar(T, float(stray[0, 0] - T[0, 3]) + 5.0, 0.0, 0.0)]
    return dict(both=both, scan=scan, poses=np.array(poses))


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_cut_index_refuses_exactly_the_poses_the_single_call_refuses(gpu, cut_world, method):
    w = cut_world
    reg = LoamRegister() if method == "loam" else VgicpRegister()
    reg.setTarget(w["both"])
    for gate in (1.0, DBL_MAX):
        s, n = reg.fitnessBatch(w["scan"], w["poses"], gate)
        refused = 0
        for k, T in enumerate(w["poses"]):
            try:
                single = reg.fitnessGated(w["scan"], T, gate)
            except PcrError as e:
                assert "cut" in str(e), str(e)
                assert (s[k], n[k]) == (-1.0, -1), (method, gate, k, s[k], n[k])
                refused += 1
                continue
            assert (s[k], int(n[k])) == single, (method, gate, k)
            _assert_batch((s[k:k + 1], n[k:k + 1]), w["scan"], w["both"], w["poses"][k:k + 1], gate, 0, (method, gate, k))
        assert refused < len(w["poses"]), "every pose refused: the test shows nothing"


def test_repeatable_and_sliced_launches_agree(gpu, scored_world):
    """70 000 poses on a 512-point subset (several internal launches): two calls return identical bytes, and slices of the poses give the
    same numbers as the whole"""
    w = scored_world
    reg = LoamRegister()
    reg.setTarget(w["map"])
    rng = np.random.default_rng(4)
    K = 70_000
    base = w["truth"]
    poses = np.repeat(base[None], K, axis=0)
    poses[:, 0, 3] += rng.uniform(-3, 3, K)
    poses[:, 1, 3] += rng.uniform(-3, 3, K)
    a = rng.uniform(-0.5, 0.5, K)
    c, s_ = np.cos(a), np.sin(a)
    R0, R1 = base[0, :3].copy(), base[1, :3].copy()
    poses[:, 0, :3] = c[:, None] * R0 - s_[:, None] * R1
    poses[:, 1, :3] = s_[:, None] * R0 + c[:, None] * R1
    s1, n1 = reg.fitnessBatch(w["scan"], poses, 1.0, 512)
    s2, n2 = reg.fitnessBatch(w["scan"], poses, 1.0, 512)
    assert s1.tobytes() == s2.tobytes() and n1.tobytes() == n2.tobytes()
    parts = [reg.fitnessBatch(w["scan"], poses[a:a + 9_999], 1.0, 512) for a in range(0, K, 9_999)]
    assert np.concatenate([p[0] for p in parts]).tobytes() == s1.tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == n1.tobytes()
    assert (n1 > 0).sum() > K // 4
    _assert_batch((s1[::7001], n1[::7001]), w["scan"], w["map"], poses[::7001], 1.0, 512, "sampled")


def test_refused_on_sharded_or_tiled_handles_and_bad_arguments(gpu, scored_world):
    w = scored_world
    reg = LoamRegister()
    with pytest.raises(PcrError, match="no target"):
        reg.fitnessBatch(w["scan"], w["poses"][:2])
    reg.setTarget(w["map"])
    reg.set_query_tile([-1e9] * 3, [1e9] * 3)
    with pytest.raises(PcrError, match="query tile"):
        reg.fitnessBatch(w["scan"], w["poses"][:2])
    with pytest.raises(PcrError, match="query tile"):
        reg.relocalize(w["scan"], w["truth"].copy())
    reg.set_query_tile(np.array([1.0, 0, 0]), np.zeros(3))      # lo > hi clears it
    assert reg.fitnessBatch(w["scan"], w["poses"][:2])[1].shape == (2,)
    with pytest.raises(PcrError, match="PCR_RELOC_MAX_POSES"):
        reg._check(reg._lib.pcr_fitness_batch(reg._h, None, 0, 16, 0, w["poses"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              (1 << 20) + 1, 1.0, 0, None, None))
    sharded = LoamRegister()
    sharded.setTarget(w["map"])
    sharded.comm_init_host(lambda ptr, count, op, user: 0, 0, 1)      # a one-rank collective: the handle is sharded
    with pytest.raises(PcrError, match="sharded"):
        sharded.fitnessBatch(w["scan"], w["poses"][:2])
    with pytest.raises(PcrError, match="sharded"):
        sharded.relocalize(w["scan"], w["truth"].copy())


# ---- pcr_relocalize ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ndt_world():
    """a denser map (0.2 m spacing) for NDT's 1 m voxels"""
    world, m = synth.make_map(300_000, seed=20261003 + 1, spacing=0.2)
    scan, T = synth.make_scan(world, 0, seed=20261003 + 1)
    return dict(world=world, map=m, scan=scan, truth=T)


OFFSETS = [(1.4, -1.1, 20.0), (-1.6, 1.3, -24.0), (1.9, 1.8, 28.0)]


def _click_that_align_misses(cls, scan, m, T):
    """the first planar offset from which a plain align ends more than 0.2 m or 2 degrees from the truth"""
    for dx, dy, yaw in OFFSETS:
        click = _planar(T, dx, dy, yaw)
        reg = cls()
        reg.setTarget(m)
        p = click.copy()
        reg.align(scan, p)
        et, er = synth.pose_error(p, T)
        if et > 0.2 or er > math.radians(2.0):
            return click, p
    pytest.fail("plain align recovered from every offset of the default window")


@pytest.mark.parametrize("method", ["loam", "vgicp", "ndt"])
def test_relocalize_end_to_end(gpu, world_100k, ndt_world, method):
    cls = {"loam": LoamRegister, "vgicp": VgicpRegister, "ndt": NdtRegister}[method]
    w = ndt_world if method == "ndt" else world_100k
    scan, m, T = w["scan"], w["map"], w["truth"]
    click, aligned = _click_that_align_misses(cls, scan, m, T)
    reg = cls()
    reg.setTarget(m)
    pose = click.copy()
    conv, cands, chosen = reg.relocalize(scan, pose)
    et, er = synth.pose_error(pose, T)
    assert et <= 0.05 and er <= math.radians(0.5), (method, et, math.degrees(er), cands)
    np.testing.assert_array_equal(pose, cands[chosen]["pose"])
    assert conv == cands[chosen]["converged"]
    # never worse than plain align from the click, under the same full-scan score
    s_al, n_al = reg.fitnessGated(scan, aligned, 1.0)
    assert cands[chosen]["n_in"] >= n_al, (cands[chosen]["n_in"], n_al)
    assert any(c["hypothesis"] == 1053 // 2 for c in cands)      # the click is a candidate
    # internals: the coarse scores are fitnessBatch of the restated lattice on the restated subset
    lattice, _, _ = restated(click, 2.0, 0.5, math.radians(30.0), math.radians(5.0))
    cs, cn = reg.fitnessBatch(scan, lattice, 1.0, 4096)
    ranked = sorted((i for i in range(len(cn)) if cn[i] > 0), key=lambda i: (-cn[i], cs[i], i))
    for c in cands:
        h = c["hypothesis"]
        assert (c["coarse_score"], c["coarse_n_in"]) == (cs[h], cn[h]), (h, c)
    assert cands[0]["hypothesis"] == ranked[0]
    # each refined pose is align from its hypothesis pose on a fresh handle with the same target, bit for bit
    fresh = cls()
    fresh.setTarget(m)
    for c in cands:
        p = lattice[c["hypothesis"]].copy()
        assert fresh.align(scan, p) == c["converged"]
        np.testing.assert_array_equal(p, c["pose"], err_msg=str(c["hypothesis"]))
    fs, fn = reg.fitnessBatch(scan, np.array([c["pose"] for c in cands]), 1.0, 0)
    assert [(c["score"], c["n_in"]) for c in cands] == list(zip(fs, fn))


def test_fitness_score_after_relocalize_is_the_chosen_poses(gpu, world_100k):
    """getFitnessScore (pcr_fitness, VGICP) right after relocalize scores the pose relocalize returned: the number a fresh align from the
    chosen hypothesis leaves -- not the last refined candidate's (the click's, appended last)"""
    w = world_100k
    scan, m, T = w["scan"], w["map"], w["truth"]
    click = _planar(T, 1.4, -1.1, 20.0)
    reg = VgicpRegister()
    reg.setTarget(m)
    pose = click.copy()
    _, cands, chosen = reg.relocalize(scan, pose)
    assert chosen != len(cands) - 1, (chosen, len(cands))      # the case where the last alignment is not the chosen one
    got = reg.getFitnessScore()
    fresh = VgicpRegister()
    fresh.setTarget(m)
    p = reloc_hypotheses(click)[cands[chosen]["hypothesis"]].copy()
    fresh.align(scan, p)
    np.testing.assert_array_equal(p, pose)
    want = fresh.getFitnessScore()
    assert got == want, (got, want)
    last = VgicpRegister()
    last.setTarget(m)
    q = reloc_hypotheses(click)[cands[-1]["hypothesis"]].copy()
    last.align(scan, q)
    assert last.getFitnessScore() != got      # (the two poses differ, and so do their scores: the test tells them apart)
    np.testing.assert_allclose(got, fr.fitness_score(scan, m, pose), rtol=fr.sum_order_rtol(len(scan)), atol=0)


def test_batch_refuses_more_points_than_it_can_hold(gpu, scored_world):
    """more than PCR_BATCH_MAX_POINTS scored per pose is refused before the source is read; a subset of a larger n_src is not"""
    w = scored_world
    reg = LoamRegister()
    reg.setTarget(w["map"])
    dp = ctypes.POINTER(ctypes.c_double)
    one = w["poses"][:1].transpose(0, 2, 1).copy()
    s, n = np.zeros(1), np.zeros(1, np.int64)
    src = np.zeros((4, 4), np.float32)
    call = lambda n_src, sp: reg._lib.pcr_fitness_batch(reg._h, src.ctypes.data_as(ctypes.c_void_p), n_src, 16, 0, one.ctypes.data_as(dp), 1, 1.0,
                                                         sp, s.ctypes.data_as(dp), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    for n_src, sp in (((1 << 26) + 1, 0), ((1 << 27), (1 << 26) + 1)):
        assert call(n_src, sp) != 0
        assert "PCR_BATCH_MAX_POINTS" in reg._lib.pcr_last_error(reg._h).decode()
    assert call(4, 0) == 0 and n[0] == fr.gated_from_sq(_ref_d2(src, w["map"], w["poses"][0]), 1.0)[1]


def test_relocalize_far_off_the_map_fails_with_a_message(gpu, world_100k):
    w = world_100k
    reg = LoamRegister()
    reg.setTarget(w["map"])
    pose = _planar(w["truth"], 500.0, 0.0, 0.0)
    before = pose.copy()
    with pytest.raises(PcrError, match="no hypothesis"):
        reg.relocalize(w["scan"], pose)
    np.testing.assert_array_equal(pose, before)


def test_loc_harness_reloc_prints_the_python_pose(gpu, world_100k, tmp_path):
    """`loc_harness params.json scan.pcd click.txt --no-downsample --reloc 2 30`: StaticMapRegister::relocalize on a PCD map, the same pose as
    the Python relocalize to 17 significant digits"""
    from tests import loc_inputs
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "loc_harness")
    w = world_100k
    click = _planar(w["truth"], 1.4, -1.1, 20.0)
    loc_inputs.write_pcd(tmp_path / "map.pcd", w["map"], "binary_pcl")
    loc_inputs.write_pcd(tmp_path / "scan.pcd", w["scan"], "binary")
    loc_inputs.write_params(tmp_path / "params.json", tmp_path / "map.pcd", pcr="loam", cores=1, grid=0.5)
    np.savetxt(tmp_path / "click.txt", click, fmt="%.17g")
    out = subprocess.run([exe, str(tmp_path / "params.json"), str(tmp_path / "scan.pcd"), str(tmp_path / "click.txt"), "--no-downsample",
                          "--reloc", "2", "30"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("pcr loam  reloc  map 100000  scan 65536"), lines[0]
    pose_cpp = np.array([[float(v) for v in ln.split()] for ln in lines[-4:]])
    reg = LoamRegister()
    reg.setTarget(w["map"])
    pose_py = click.copy()
    _, cands, chosen = reg.relocalize(w["scan"], pose_py, xy_range=2.0, yaw_range=math.radians(30.0))
    assert lines[-5].startswith(f"chosen {chosen} hypothesis {cands[chosen]['hypothesis']} "), lines[-5]
    want = [" ".join(f"{v:.17g}" for v in row) for row in pose_py]
    assert lines[-4:] == want, (lines[-4:], want)
    np.testing.assert_array_equal(pose_cpp, pose_py)
