"""The gicp method on the GPU (csrc/gicp.hip, gicp_host.hip) against the plain reference tests/gicp_ref.py: correspondences index for index
and distance bit for bit, Mahalanobis matrices and sums within gicp_ref.DEVICE_*_BOUND, whole alignments against gicp_ref.align."""
import os
import subprocess

import numpy as np
import pytest

import fitness_ref
import gicp_ref
import oracle
from simpleslam_amd import GicpRegister, PcrError, SubMap, make_register, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def w():
    return gicp_ref.world_small_case()


@pytest.fixture(scope="module")
def kept(gpu, w):
    """one register with world_small's map as its kept target"""
    reg = GicpRegister()
    reg.setTarget(w["map"])
    return reg


def check_linearisation(got, ref, what, sums=True):
    """corr and d2 exactly on every non-ambiguous point (the reference's ambiguous share is asserted below 1 % first), n_corr exactly when no
    point is ambiguous, M, H, b, err within the device bounds (each figure printed before it is asserted)"""
    amb = ref["ambiguous"]
    assert amb.sum() < 0.01 * max(amb.size, 1), (what, int(amb.sum()))
    ok = ~amb
    np.testing.assert_array_equal(got["corr"][ok], ref["corr"][ok], err_msg=what)
    np.testing.assert_array_equal(got["d2"][ok].view(np.uint32), ref["d2"][ok].view(np.uint32), err_msg=what)
    if not amb.any():
        assert got["n"] == ref["n"], what
    if not sums:
        return
    same = ok & (got["corr"] == ref["corr"])
    dM = gicp_ref.m_diff(got["M"][same], ref["M"][same])
    dH, db, de = gicp_ref.sums_diff(got, ref)
    print(what, "n %d  M %.3g  H %.3g  b %.3g  err %.3g" % (ref["n"], dM, dH, db, de))
    assert dM <= gicp_ref.DEVICE_M_BOUND, (what, dM)
    assert dH <= gicp_ref.DEVICE_H_BOUND and db <= gicp_ref.DEVICE_B_BOUND and de <= gicp_ref.DEVICE_ERR_BOUND, (what, dH, db, de)


@pytest.mark.parametrize("at", ["init", "truth"])
def test_correspondences_and_sums_at_two_poses(kept, w, at):
    pose, other = w[at], w["truth" if at == "init" else "init"]
    ref = gicp_ref.linearize(w["scan"], w["map"], pose, w["C_A"], w["C_B"], with_ambiguous=True)
    got = kept.linearize(w["scan"], pose, pose_eval=other, per_point=True)
    check_linearisation(got, ref, at)
    want = gicp_ref.error(w["scan"], w["map"], other, ref["corr"], ref["M"])
    de = abs(got["err_eval"] - want) / abs(want)
    print(at, "err_eval %.3g" % de)
    assert de <= gicp_ref.DEVICE_ERR_BOUND, de


def test_the_gate(gpu, w):
    ref = gicp_ref.linearize(w["scan"], w["map"], w["init"], w["C_A"], w["C_B"], 0.3, with_ambiguous=True)
    assert 0 < ref["n"] < w["scan"].shape[0]
    reg = GicpRegister(gicp_max_corr_dist=0.3)
    reg.setTarget(w["map"])
    got = reg.linearize(w["scan"], w["init"], per_point=True)
    np.testing.assert_array_equal(got["corr"] == -1, ref["corr"] == -1)
    assert np.isinf(got["d2"][got["corr"] == -1]).all()
    check_linearisation(got, ref, "gate 0.3")


def test_exact_ties_go_to_the_lower_index(gpu):
    src, dst, want = gicp_ref.lattice_case()
    reg = GicpRegister()
    reg.setTarget(dst)
    got = reg.linearize(src, np.eye(4), per_point=True)
    np.testing.assert_array_equal(got["corr"], want)
    assert (got["d2"] == np.float32(0.25)).all()
    reg.setTarget(dst[::-1].copy())                              # rows reversed: the other end of every edge is the lower index now
    np.testing.assert_array_equal(reg.linearize(src, np.eye(4), per_point=True)["corr"], 215 - (want + 36))


def test_more_than_65536_source_points(gpu):
    """70 000 source points are 274 blocks of 256: more than the 256 rows the prologue of the device loop folds in its first round, and more
    than one round of the stand-alone fold"""
    world, m = synth.make_map(5_000, seed=6)
    scan, T = synth.make_scan(world, 0, seed=6, beams=35, azimuths=2000)
    assert scan.shape[0] == 70_000
    init = synth.perturb(T, 6, trans=0.2, rot_deg=1.0)
    CA, CB = oracle.vgicp_covariances(scan, threads=8), oracle.vgicp_covariances(m, threads=8)
    ref = gicp_ref.linearize(scan, m, init, CA, CB, with_ambiguous=True)
    reg = GicpRegister()
    reg.setTarget(m)
    got = reg.linearize(scan, init, per_point=True)
    check_linearisation(got, ref, "70 000 x 5 000")
    # ... and the device-resident loop's fold of those rows decides as the host-driven loop's
    host = GicpRegister(host_optimiser=1)
    host.setTarget(m)
    pd, ph = init.copy(), init.copy()
    assert reg.align(scan, pd) == host.align(scan, ph)
    assert reg.stats()["iterations"] == host.stats()["iterations"]
    dt, dr = synth.pose_error(pd, ph)
    assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)


def test_edges(gpu, kept, w):
    I = np.eye(4)
    # no source point
    got = kept.linearize(np.zeros((0, 4), np.float32), I, per_point=True)
    assert got["n"] == 0 and not got["H"].any() and not got["b"].any() and got["err"] == 0.0
    # NaN and inf points in the target do not renumber the others; NaN points in the source have no correspondence; one block of < 256 points
    m = w["map"][:4000].copy()
    m[[5, 777, 3999], 0] = [np.nan, np.inf, -np.inf]
    src = w["scan"][:200].copy()
    src[[3, 150], 1] = np.nan
    finite = np.isfinite(m[:, :3]).all(axis=1)
    CB = np.zeros((m.shape[0], 3, 3))
    CB[finite] = oracle.vgicp_covariances(m[finite], threads=8)
    ref = gicp_ref.linearize(src, m, w["truth"], w["C_A"][:200], CB, with_ambiguous=True)
    assert (ref["corr"][[3, 150]] == -1).all() and ref["n"] == 198 and not np.isin(ref["corr"], [5, 777, 3999]).any()
    reg = GicpRegister()
    reg.setTarget(m)
    got = reg.linearize(src, w["truth"], per_point=True)
    check_linearisation(got, ref, "edges", sums=False)           # (the first 200 points' own covariances are another cloud's: only the pairs here)
    assert (got["corr"][[3, 150]] == -1).all()


def test_scan2map_equals_the_reference_alignment(gpu, w):
    a = gicp_ref.world_small_alignment()
    reg = GicpRegister()
    pose = w["init"].copy()
    conv = reg.scan2Map(w["scan"], w["map"], pose)
    assert conv == a["converged"] and reg.stats()["iterations"] == a["outer"]
    dt, dr = synth.pose_error(pose, a["pose"])
    print("scan2Map vs gicp_ref.align: %.3g m %.3g rad" % (dt, dr))
    assert dt <= 1e-4 and dr <= 1e-4
    want = fitness_ref.fitness_score(w["scan"], w["map"], pose)
    np.testing.assert_allclose(reg.getFitnessScore(), want, rtol=fitness_ref.sum_order_rtol(w["scan"].shape[0]), atol=0)


def test_device_resident_optimiser_equals_the_host_driven_one(gpu, w):
    """the assertions test_vgicp_gpu.py makes for vgicp's two loops, and identical bytes from identical calls"""
    dev, host = GicpRegister(), GicpRegister(host_optimiser=1)
    for seed, tr, rd in ((41, 0.3, 2.0), (42, 0.1, 0.5), (43, 0.6, 4.0), (44, 0.0, 0.0), (45, 1.5, 8.0)):
        T0 = synth.perturb(w["truth"], seed, trans=tr, rot_deg=rd) if tr else w["truth"].copy()
        pd, ph = T0.copy(), T0.copy()
        assert dev.scan2Map(w["scan"], w["map"], pd) == host.scan2Map(w["scan"], w["map"], ph), seed
        sd, sh = dev.stats(), host.stats()
        assert (sd["iterations"], sd["kernel_launches"]) == (sh["iterations"], sh["kernel_launches"]), (seed, sd, sh)
        dt, dr = synth.pose_error(pd, ph)
        print("seed %d: %d iterations, device against host loop %.3g m %.3g rad" % (seed, sd["iterations"], dt, dr))
        assert dt <= 2e-6 and dr <= 2e-6, (seed, dt, dr)      # (a float ulp of the pose at 10 m is 1e-6)
        np.testing.assert_allclose(dev.getFitnessScore(), host.getFitnessScore(), rtol=1e-5)
    first = w["init"].copy(); dev.scan2Map(w["scan"], w["map"], first)
    for _ in range(20):
        p = w["init"].copy(); dev.scan2Map(w["scan"], w["map"], p)
        np.testing.assert_array_equal(p, first)
    for cap in (1, 2, 3):
        ra, rb = GicpRegister(vgicp_max_iters=cap), GicpRegister(vgicp_max_iters=cap, host_optimiser=1)
        qa, qb = w["init"].copy(), w["init"].copy()
        assert ra.scan2Map(w["scan"], w["map"], qa) == rb.scan2Map(w["scan"], w["map"], qb)
        assert ra.stats()["iterations"] == rb.stats()["iterations"] == cap
        dt, dr = synth.pose_error(qa, qb)
        assert dt <= 2e-6 and dr <= 2e-6, (cap, dt, dr)


@pytest.fixture(scope="module")
def keyframes():
    world, _ = synth.make_map(20_000, seed=91)
    kfs = []
    for j in range(12):
        scan, T = synth.make_scan(world, j, seed=91, beams=32, azimuths=512)
        kfs.append((oracle.voxel_filter(scan, 0.4)[0], T))
    return world, kfs


def test_kept_target(gpu, w, keyframes):
    scans = [w["scan"], np.ascontiguousarray(w["scan"][::2])]
    reg = GicpRegister()
    reg.setTarget(w["map"])
    for k, scan in enumerate(scans):
        init = synth.perturb(w["truth"], 60 + k, trans=0.2, rot_deg=1.0)
        p_keep, p_fresh = init.copy(), init.copy()
        fresh = GicpRegister()
        fresh.setTarget(w["map"])
        assert reg.align(scan, p_keep) == fresh.align(scan, p_fresh)
        np.testing.assert_array_equal(p_keep, p_fresh)
        p_s2m = init.copy()
        GicpRegister().scan2Map(scan, w["map"], p_s2m)
        np.testing.assert_array_equal(p_keep, p_s2m)
    # a SubMap as the target: built once per generation, the pose of pcr_scan2map_device on the same memory
    world, kfs = keyframes
    sm = SubMap()
    for c, T in kfs[:9]:
        sm.addKeyFrame(c, T)
    sm.updateMap(kfs[9][1][:3, 3], radius=8.0, grid_size=0.4)
    reg, ref = GicpRegister(), GicpRegister()
    for k in (9, 10):
        ds = reg.voxelDownSample(kfs[k][0], 0.4)
        init = synth.perturb(kfs[k][1], 91 + k, trans=0.1, rot_deg=0.5)
        p_keep, p_ref = init.copy(), init.copy()
        assert reg.scan2MapSubmap(ds, sm, p_keep) == ref.scan2MapSubmap(ds, sm, p_ref, rebuild=True)
        np.testing.assert_array_equal(p_keep, p_ref)
    assert reg.stats()["target_builds"] == 1
    sm.updateMap(kfs[10][1][:3, 3], radius=8.0, grid_size=0.4)
    p_keep, p_ref = init.copy(), init.copy()
    reg.scan2MapSubmap(ds, sm, p_keep)
    ref.scan2MapSubmap(ds, sm, p_ref, rebuild=True)
    np.testing.assert_array_equal(p_keep, p_ref)
    assert reg.stats()["target_builds"] == 2


def test_kept_target_outlives_the_callers_device_buffer(gpu, w, keyframes):
    """pcr_scan2map_device leaves the target kept, and every pass reads target points at their original index: from the handle's own copy,
    so the caller may overwrite or free its tensor before the next pcr_align or pcr_gicp_linearize"""
    import torch
    d_scan, d_map = torch.from_numpy(w["scan"].copy()).cuda(), torch.from_numpy(w["map"].copy()).cuda()
    reg = GicpRegister()
    first = w["init"].copy()
    reg.scan2Map(d_scan, d_map, first)
    d_map.zero_()
    torch.cuda.synchronize()
    del d_map
    fresh = GicpRegister()
    fresh.setTarget(w["map"])
    init = synth.perturb(w["truth"], 61, trans=0.2, rot_deg=1.0)
    p_kept, p_fresh = init.copy(), init.copy()
    assert reg.align(d_scan, p_kept) == fresh.align(d_scan, p_fresh)
    np.testing.assert_array_equal(p_kept, p_fresh)
    a, b = reg.linearize(w["scan"], w["truth"]), fresh.linearize(w["scan"], w["truth"])
    np.testing.assert_array_equal(a["H"], b["H"])
    assert (a["err"], a["n"]) == (b["err"], b["n"])
    # a sub-map that moves on under a handle which is then used through pcr_align: the target is still the generation it was prepared from
    world, kfs = keyframes
    sm = SubMap()
    for c, T in kfs:
        sm.addKeyFrame(c, T)
    sm.updateMap(kfs[3][1][:3, 3], radius=8.0, grid_size=0.4)
    old = sm.download()
    ds = reg.voxelDownSample(kfs[3][0], 0.4)
    g = synth.perturb(kfs[3][1], 93, trans=0.1, rot_deg=0.5)
    tmp = g.copy()
    reg.scan2MapSubmap(ds, sm, tmp)
    sm.updateMap(kfs[10][1][:3, 3], radius=3.0, grid_size=0.4)
    pa, pb = g.copy(), g.copy()
    fresh.setTarget(old)
    assert reg.align(ds, pa) == fresh.align(ds, pb)
    np.testing.assert_array_equal(pa, tmp)
    np.testing.assert_array_equal(pa, pb)


def test_init_for_lc_against_a_window_of_a_view(gpu, keyframes):
    world, kfs = keyframes
    sm = SubMap()
    for c, T in kfs:
        sm.addKeyFrame(c, T)
    lc_map = sm.view()
    key, rng = 6, 2
    lc_map.loopFindNearKeyframes(key, rng, grid_size=0.4)
    scan, T_true = kfs[key]
    guess = synth.perturb(T_true, 7, trans=0.3, rot_deg=1.5)      # the loop-closure-sized error of test_submap_gpu.py
    lc = GicpRegister()
    lc.initForLC()
    assert (lc.params.vgicp_max_iters, lc.params.vgicp_trans_eps, lc.params.gicp_max_corr_dist) == (100, 1e-6, 150.0)
    pose = guess.copy()
    conv = lc.scan2MapSubmap(scan, lc_map, pose)
    et, er = synth.pose_error(pose, T_true)
    print("loop closure: %.3g m %.3g rad, fitness %.3g" % (et, er, lc.getFitnessScore()))
    assert conv and et < 0.05 and er < 5e-3
    born = GicpRegister(vgicp_max_iters=100, vgicp_trans_eps=1e-6, gicp_max_corr_dist=150.0)
    pose_b = guess.copy()
    assert born.scan2MapSubmap(scan, lc_map, pose_b) == conv
    np.testing.assert_array_equal(pose, pose_b)


def test_refusals_name_gicp_and_leave_the_handle_usable(gpu, w):
    reg = GicpRegister()
    lo, hi = np.array([-10.0, -10.0, -10.0]), np.array([10.0, 10.0, 10.0])
    for call in (lambda: reg.set_shard(lo, hi, 4.0), lambda: reg.set_query_tile(lo, hi), lambda: reg.comm_init_host(lambda p, n, op, u: 0, 0, 2)):
        with pytest.raises(PcrError, match="gicp"):
            call()
    m = w["map"].copy()
    m[0, :3] = [30000.0, -25000.0, 8000.0]                      # a stray point 40 km away: a box no dense table holds
    for call in (lambda: reg.setTarget(m), lambda: reg.scan2Map(w["scan"], m, w["init"].copy())):
        with pytest.raises(PcrError, match="gicp"):
            call()
    pose, want = w["init"].copy(), w["init"].copy()
    conv = reg.scan2Map(w["scan"], w["map"], pose)
    assert GicpRegister().scan2Map(w["scan"], w["map"], want) == conv
    np.testing.assert_array_equal(pose, want)


def test_cpp_mirror_takes_gicp_from_params_json(gpu, w, tmp_path):
    from tests import loc_inputs
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "loc_harness")
    loc_inputs.write_pcd(tmp_path / "map.pcd", w["map"], "binary")
    loc_inputs.write_pcd(tmp_path / "scan.pcd", w["scan"], "binary")
    loc_inputs.write_params(tmp_path / "params.json", tmp_path / "map.pcd", pcr="gicp", cores=1, grid=0.5)
    np.savetxt(tmp_path / "init.txt", w["init"], fmt="%.17g")
    out = subprocess.run([exe, str(tmp_path / "params.json"), str(tmp_path / "scan.pcd"), str(tmp_path / "init.txt"), "--no-downsample"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("pcr gicp "), out.stdout[:80]
    pose_cpp = np.array([[float(v) for v in ln.split()] for ln in out.stdout.strip().splitlines()[-4:]])
    pose_py = w["init"].copy()
    conv = make_register("gicp").scan2Map(w["scan"], w["map"], pose_py)
    assert f"converged {int(conv)}" in out.stdout.splitlines()[0]
    np.testing.assert_array_equal(pose_cpp, pose_py)
