"""fast_gicp's regularisation methods and voxel accumulation modes on the device (pcr_params.vgicp_regularization, vgicp_voxel_mode) against
tests/gicp_settings_ref.py: the covariances on both kernel paths, the voxel fold per voxel (pcr_vgicp_voxels), its accumulator's range, one
linearisation, and the life cycle of the two parameters.  Every bound is ten times a figure the reference shows against a second evaluation
of itself (tests/test_gicp_settings_ref.py), plus 2^-45 where the fixed-scale fold quantises; each test prints what it observed."""
import numpy as np
import pytest

import cov_ref
import gicp_ref
import gicp_settings_ref as R
from simpleslam_amd import GicpRegister, VgicpRegister, shard, synth

pytestmark = pytest.mark.gpu

SCAN_NAMES = ["blob", "lidar", "plane", "two_planes", "clump"]
REGS = (R.NONE, R.MIN_EIG, R.NORMALIZED_MIN_EIG, R.PLANE, R.FROBENIUS)


def _pairs():
    """every (regularisation, voxel mode): all are well conditioned on fold_map() (asserted on the reference by the CPU suite and below)"""
    return [(reg, mode) for reg in REGS for mode in (R.ADDITIVE, R.MULTIPLICATIVE)]


# ---------------------------------------------------------------------------
# 1. covariances, scan-sized path
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_refs():
    return {name: R.scatter(cov_ref.clouds()[name]) for name in SCAN_NAMES}


@pytest.mark.parametrize("name", SCAN_NAMES)
def test_scan_sized_covariances(gpu, scan_refs, name):
    pts = cov_ref.clouds()[name]
    S, ref = scan_refs[name]
    keep = ~ref.ambiguous
    assert ref.ambiguous.mean() < 0.01
    queued_any = 0
    for reg in R.NEW_REGS:
        h = VgicpRegister(vgicp_regularization=reg)
        got = h.covariances(pts)
        nb, queued = h.neighbours(len(pts))
        queued_any += queued
        assert (nb[keep] == ref.idx[keep]).all()      # the lists do not depend on the regularisation
        d = R.rel_diff(got, R.regularize(S, reg))
        print(f"{name} {R.REG_NAMES[reg]}: max {d[keep].max():.3e} (bound {R.DEVICE_REG_BOUND[reg]:.1e}), wave kernel {queued} of {len(pts)}")
        assert np.isfinite(got).all() and np.array_equal(got, got.transpose(0, 2, 1))
        over = keep & ~(d <= R.DEVICE_REG_BOUND[reg])
        assert not over.any(), (name, R.REG_NAMES[reg], int(over.sum()), float(d[keep].max()), np.flatnonzero(over)[:8])
    if name == "clump":
        assert queued_any > 0      # (thousands of candidates per query: the wave kernel ran)


def test_a_gicp_handle_reads_the_regularisation(gpu, scan_refs):
    pts = cov_ref.clouds()["blob"]
    a = VgicpRegister(vgicp_regularization=R.FROBENIUS).covariances(pts)
    b = GicpRegister(vgicp_regularization=R.FROBENIUS, vgicp_voxel_mode=R.MULTIPLICATIVE).covariances(pts)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# 2. covariances, map-sized path
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def map_case(gpu):
    m, clusters = cov_ref.cluster_map()
    assert 300_000 < len(m) <= 303_000
    return dict(map=m, clusters=clusters, cov={reg: VgicpRegister(vgicp_regularization=reg).covariances(m) for reg in R.NEW_REGS})


def test_map_sized_covariances_match_the_reference(map_case):
    """FROBENIUS (two inverses and a norm: the most arithmetic) on 40 sampled queries of each of the first nine clusters, brute-forced inside
    their cluster, which the asserted separation makes the whole cloud's answer"""
    m, rng, worst, n = map_case["map"], np.random.default_rng(63), 0.0, 0
    for q, (kind, a, b) in enumerate(map_case["clusters"][:9]):
        rows = np.sort(rng.choice(b - a, 40, replace=False))
        S, ref = R.scatter(m[a:b], rows)
        assert (np.sqrt(ref.d2[:, 20].astype(np.float64)) < cov_ref.distance_to_other_clusters(m[a:b][rows], q)).all(), (q, kind)
        keep = ~ref.ambiguous
        d = R.rel_diff(map_case["cov"][R.FROBENIUS][a + rows], R.regularize(S, R.FROBENIUS))
        assert (d[keep] <= R.DEVICE_REG_BOUND[R.FROBENIUS]).all(), (kind, float(d[keep].max()))
        worst, n = max(worst, float(d[keep].max())), n + int(keep.sum())
    print(f"map-sized FROBENIUS: max {worst:.3e} over {n} queries (bound {R.DEVICE_REG_BOUND[R.FROBENIUS]:.1e})")
    assert n >= 350


@pytest.mark.parametrize("reg", R.NEW_REGS)
def test_the_two_paths_give_the_same_bits(map_case, reg):
    """a cluster inside the map-sized cloud (vgicp_cov_kernel<false>) and alone (cov_search.hip): one arithmetic (cov_math.h), the same bits"""
    m, checked = map_case["map"], 0
    for q, (kind, a, b) in enumerate(map_case["clusters"][:4]):
        alone = VgicpRegister(vgicp_regularization=reg).covariances(np.ascontiguousarray(m[a:b]))
        _, d2 = cov_ref.neighbours(m[a:b])
        inside = np.sqrt(d2[:, 20].astype(np.float64)) < cov_ref.distance_to_other_clusters(m[a:b], q)
        assert inside.mean() > 0.99, (kind, inside.mean())
        differ = (alone != map_case["cov"][reg][a:b]).any(axis=(1, 2)) & inside
        assert not differ.any(), (kind, int(differ.sum()), np.flatnonzero(differ)[:8])
        checked += int(inside.sum())
    assert checked > 7_000


# ---------------------------------------------------------------------------
# 3. / 4. the voxel fold, per voxel
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold_case():
    m = cov_ref.fold_map()
    s = cov_ref.fold_scan(m)
    Sm, rm = R.scatter(m)
    Ss, rs = R.scatter(s)
    assert not rm.ambiguous.any() and not rs.ambiguous.any() and (np.diff(rm.d2, axis=1) > 0).all()      # lists independent of the rows' order
    assert R.conditioning(Sm).min() >= R.COND_FLOOR and R.conditioning(Ss).min() >= R.COND_FLOOR
    return dict(map=m, scan=s, Sm=Sm, Ss=Ss, perm=np.random.default_rng(62).permutation(len(m)))


def _check_voxels(got, want, reg, mode, label):
    assert np.array_equal(got["ijk"], want["ijk"]) and np.array_equal(got["n"], want["n"]), label
    bm, bc = R.DEVICE_FOLD_BOUND[(reg, mode)]
    q = R.FIXED_FOLD_QUANTUM if (reg, mode) in R.FIXED_FOLD else 0.0
    sm, sc = np.abs(want["mean"]).max(axis=1), np.abs(want["cov"]).max(axis=(1, 2))
    em, ec = np.abs(got["mean"] - want["mean"]).max(axis=1), np.abs(got["cov"] - want["cov"]).max(axis=(1, 2))
    print(f"{label}: {len(sm)} voxels, largest {want['n'].max()} points, mean {np.max(em / sm):.3e} (bound {bm:.1e}), cov {np.max(ec / sc):.3e} (bound {bc:.1e}), "
          f"quantum {q:.1e}, largest entry {sc.max():.3e}")
    assert np.isfinite(got["cov"]).all() and np.isfinite(got["mean"]).all(), label
    assert (em <= bm * sm + q).all(), (label, float(np.max(em / sm)))
    assert (ec <= bc * sc + q).all(), (label, float(np.max(ec / sc)))


def _same_records(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ijk", "n", "mean", "cov"))


@pytest.mark.parametrize("res", [1.0, 2.0])
@pytest.mark.parametrize("reg,mode", _pairs())
def test_voxel_fold_per_voxel(gpu, fold_case, reg, mode, res):
    m = fold_case["map"]
    cnt = cov_ref.voxel_counts(m, res)
    assert (cnt * max(res, 1.0) > 256).any() and (cnt * max(res, 1.0) <= 256).any()      # both accumulators of the fixed-scale fold
    want = R.fold(m, R.regularize(fold_case["Sm"], reg), res, mode)
    h = VgicpRegister(vgicp_resolution=res, vgicp_regularization=reg, vgicp_voxel_mode=mode)
    h.setTarget(m)
    got = h.voxels()
    _check_voxels(got, want, reg, mode, f"{R.REG_NAMES[reg]} {R.MODE_NAMES[mode]} res {res}")
    hp = VgicpRegister(vgicp_resolution=res, vgicp_regularization=reg, vgicp_voxel_mode=mode)
    hp.setTarget(np.ascontiguousarray(m[fold_case["perm"]]))
    assert _same_records(hp.voxels(), got)      # the order of the map's rows does not reach a bit
    if mode == R.ADDITIVE:
        h1 = VgicpRegister(vgicp_resolution=res, vgicp_regularization=reg, vgicp_voxel_mode=R.ADDITIVE_WEIGHTED)
        h1.setTarget(m)
        assert _same_records(h1.voxels(), got)


def test_voxels_of_a_region_only_target_are_refused(gpu, fold_case):
    from simpleslam_amd import PcrError
    h = VgicpRegister()
    with pytest.raises(PcrError, match="pcr_set_target first"):
        h.voxels()
    T = np.eye(4)
    h.scan2Map(fold_case["scan"], fold_case["map"], T)
    with pytest.raises(PcrError, match="pcr_set_target first"):
        h.voxels()


@pytest.mark.parametrize("reg,scale", [(R.NONE, 8.0), (R.FROBENIUS, 1.0), (R.NONE, 1024.0), (R.MIN_EIG, 1024.0)])
def test_accumulator_range(gpu, fold_case, reg, scale):
    """Terms beyond what a fixed scale of 2^44 holds.  The map scaled by a power of two at a resolution scaled alike has the same voxels and
    scatters scale^2 times as large, exactly; FROBENIUS on the map as it is has entries up to (w_max + 1e-3) / 1e-3.
    - NONE x 8 and FROBENIUS x 1 (the issue's cases): in the 1 000-point voxel cnt * max|entry| is 1.7e3 and 6.5e3, above 2^9, where the doubles
      of a fixed-scale fold stop being exact -- but a voxel of that size is folded in long long there, which holds until 2^19;
    - NONE and MIN_EIG x 1024: cnt * max|entry| is about 2.8e7 > 2^19, so cnt * max|entry| * 2^44 > 2^63 and a long long sum at the fixed scale
      wraps: only a scale chosen per voxel can pass.  (MIN_EIG leaves these scatters as they are: every eigenvalue is above 1e-3.)
    The same bound as at any other size, and the same bits whatever the order of the rows.  (MULTIPLICATIVE meets such loads in
    test_voxel_fold_per_voxel already: PLANE's inverse covariances reach 1e3, a thousand of them 1e6 > 2^19.)"""
    m = fold_case["map"].copy()
    m[:, :3] *= np.float32(scale)
    S = fold_case["Sm"] * scale * scale      # (exact: a power of four)
    covs = R.regularize(S, reg)
    want = R.fold(m, covs, scale, R.ADDITIVE)
    big = int(np.argmax(want["n"]))
    load = float(want["n"][big] * np.abs(covs[want["rows"][big]]).max())
    print(f"{R.REG_NAMES[reg]} x{scale}: voxel of {want['n'][big]} points, cnt * max|entry| = {load:.3e} (2^9 = 512, 2^19 = 524288)")
    assert want["n"][big] >= 1000 and load > 3 * 512
    if scale == 1024.0:
        assert load > 2.0 ** 19 and load * 2.0 ** 44 > 2.0 ** 63      # the fixed scale's long long sum would wrap
        assert np.abs(want["cov"][big]).max() > 2.0 ** 10              # (and the voxel's own covariance is far from a unit one)
    h = VgicpRegister(vgicp_resolution=scale, vgicp_regularization=reg)
    h.setTarget(m)
    got = h.voxels()
    _check_voxels(got, want, reg, R.ADDITIVE, f"range {R.REG_NAMES[reg]} x{scale}")
    hp = VgicpRegister(vgicp_resolution=scale, vgicp_regularization=reg)
    hp.setTarget(np.ascontiguousarray(m[fold_case["perm"]]))
    assert _same_records(hp.voxels(), got)


def test_a_term_that_is_not_finite_makes_the_voxel_nan(gpu):
    """NONE leaves the scatter of an exact plane singular (cov_ref's `plane`: z constant, the zz row exactly zero), and MULTIPLICATIVE inverts
    it: the determinant is exactly 0, the inverse holds inf and NaN.  Every voxel's covariance and mean must then be NaN -- not whatever an
    integer conversion makes of them -- with the right counts, for the rows in any order."""
    m = cov_ref.clouds()["plane"]
    S, _ = R.scatter(m)
    assert (S[:, 2, :] == 0).all()
    want_ijk, want_n = np.unique(cov_ref.voxel_coords(m[:, :3], 1.0), axis=0, return_counts=True)
    h = VgicpRegister(vgicp_regularization=R.NONE, vgicp_voxel_mode=R.MULTIPLICATIVE)
    h.setTarget(m)
    got = h.voxels()
    assert np.array_equal(got["ijk"], want_ijk) and np.array_equal(got["n"], want_n) and want_n.max() >= 16
    assert np.isnan(got["cov"]).all() and np.isnan(got["mean"]).all()
    hp = VgicpRegister(vgicp_regularization=R.NONE, vgicp_voxel_mode=R.MULTIPLICATIVE)
    hp.setTarget(np.ascontiguousarray(m[np.random.default_rng(64).permutation(len(m))]))
    gp = hp.voxels()
    assert np.array_equal(gp["ijk"], got["ijk"]) and np.array_equal(gp["n"], got["n"]) and np.isnan(gp["cov"]).all() and np.isnan(gp["mean"]).all()
    # the same cloud under ADDITIVE has nothing to invert: finite, and the zz entry exactly zero
    ha = VgicpRegister(vgicp_regularization=R.NONE)
    ha.setTarget(m)
    ga = ha.voxels()
    assert np.isfinite(ga["cov"]).all() and (ga["cov"][:, 2, 2] == 0).all()


# ---------------------------------------------------------------------------
# 5. one linearisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("reg,mode", [(R.MIN_EIG, R.ADDITIVE), (R.PLANE, R.MULTIPLICATIVE), (R.FROBENIUS, R.MULTIPLICATIVE)])
def test_vgicp_linearisation(gpu, fold_case, reg, mode):
    m, s = fold_case["map"], fold_case["scan"]
    Cs = R.regularize(fold_case["Ss"], reg)
    vox = R.fold(m, R.regularize(fold_case["Sm"], reg), 1.0, mode)
    h = VgicpRegister(vgicp_regularization=reg, vgicp_voxel_mode=mode)
    h.setTarget(m)
    bound = R.DEVICE_LIN_BOUND[(reg, mode)]
    for T in cov_ref.fold_poses():
        want, got = R.linearize(s, T, Cs, vox, 1.0), h.linearize(s, T)
        assert got["n"] == want["n"] >= 300
        d = cov_ref.lin_diff(got, want)
        print(f"{R.REG_NAMES[reg]} {R.MODE_NAMES[mode]}: n {got['n']}, H {d[0]:.3e} b {d[1]:.3e} err {d[2]:.3e} (bounds {bound})")
        assert all(x <= y for x, y in zip(d, bound)), d


@pytest.fixture(scope="module")
def world_refs():
    """gicp_ref's small world with the scatters of both clouds by brute force: computed once"""
    w = gicp_ref.world_small_case()
    Sm, rm = R.scatter(w["map"])
    Ss, rs = R.scatter(w["scan"])
    return dict(w=w, Sm=Sm, Ss=Ss, amb=int(rm.ambiguous.sum() + rs.ambiguous.sum()))


def test_gicp_linearisation_with_frobenius_covariances(gpu, world_refs):
    w = world_refs["w"]
    C_A, C_B = R.regularize(world_refs["Ss"], R.FROBENIUS), R.regularize(world_refs["Sm"], R.FROBENIUS)
    want = gicp_ref.linearize(w["scan"], w["map"], w["init"], C_A, C_B, with_ambiguous=True)
    h = GicpRegister(vgicp_regularization=R.FROBENIUS)
    h.setTarget(w["map"])
    got = h.linearize(w["scan"], w["init"], per_point=True)
    clear = ~want["ambiguous"]
    assert (got["corr"][clear] == want["corr"][clear]).all() and want["ambiguous"].mean() < 0.01
    if not want["ambiguous"].any() and world_refs["amb"] == 0:
        d = gicp_ref.sums_diff(got, want)
        print(f"gicp FROBENIUS: n {got['n']}, H {d[0]:.3e} b {d[1]:.3e} err {d[2]:.3e}")
        assert got["n"] == want["n"]
        assert d[0] <= gicp_ref.DEVICE_H_BOUND + R.DEVICE_REG_BOUND[R.FROBENIUS] and d[1] <= gicp_ref.DEVICE_B_BOUND + R.DEVICE_REG_BOUND[R.FROBENIUS]
        assert d[2] <= gicp_ref.DEVICE_ERR_BOUND + R.DEVICE_REG_BOUND[R.FROBENIUS]
    md = gicp_ref.m_diff(got["M"][clear], want["M"][clear])
    print(f"gicp FROBENIUS: M {md:.3e}")
    assert md <= gicp_ref.DEVICE_M_BOUND + R.DEVICE_REG_BOUND[R.FROBENIUS]


# ---------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------
def test_end_to_end_vgicp_min_eig_multiplicative(gpu, world_refs):
    w = world_refs["w"]
    Cs = R.regularize(world_refs["Ss"], R.MIN_EIG)
    vox = R.fold(w["map"], R.regularize(world_refs["Sm"], R.MIN_EIG), 1.0, R.MULTIPLICATIVE)
    want = R.vgicp_align(w["scan"], vox, w["init"], Cs)
    poses = []
    for host in (0, 1):
        h = VgicpRegister(vgicp_regularization=R.MIN_EIG, vgicp_voxel_mode=R.MULTIPLICATIVE, host_optimiser=host)
        T = w["init"].copy()
        conv = h.scan2Map(w["scan"], w["map"], T)
        dt, da = synth.pose_error(T, want["pose"])
        print(f"vgicp MIN_EIG MULTIPLICATIVE host_optimiser {host}: converged {conv} iterations {h.stats()['iterations']} (reference {want['converged']} {want['outer']}), "
              f"pose off by {dt:.2e} m {da:.2e} rad")
        assert conv == want["converged"] and h.stats()["iterations"] == want["outer"]
        assert dt <= 1e-4 and da <= 1e-4      # the project's parity criterion
        poses.append(T)
    dt, da = synth.pose_error(poses[0], poses[1])
    assert dt <= 2e-6 and da <= 2e-6      # (as test_device_resident_optimiser_equals_the_host_driven_one)


def test_end_to_end_gicp_normalized_min_eig(gpu, world_refs):
    w = world_refs["w"]
    C_A, C_B = R.regularize(world_refs["Ss"], R.NORMALIZED_MIN_EIG), R.regularize(world_refs["Sm"], R.NORMALIZED_MIN_EIG)
    want = R.gicp_align(w["scan"], w["map"], w["init"], C_A, C_B)
    poses = []
    for host in (0, 1):
        h = GicpRegister(vgicp_regularization=R.NORMALIZED_MIN_EIG, host_optimiser=host)
        T = w["init"].copy()
        conv = h.scan2Map(w["scan"], w["map"], T)
        dt, da = synth.pose_error(T, want["pose"])
        print(f"gicp NORMALIZED_MIN_EIG host_optimiser {host}: converged {conv} iterations {h.stats()['iterations']} (reference {want['converged']} {want['outer']}), "
              f"pose off by {dt:.2e} m {da:.2e} rad")
        assert conv == want["converged"] and h.stats()["iterations"] == want["outer"]
        assert dt <= 1e-4 and da <= 1e-4
        poses.append(T)
    dt, da = synth.pose_error(poses[0], poses[1])
    assert dt <= 2e-6 and da <= 2e-6


# ---------------------------------------------------------------------------
# 7. life cycle
# ---------------------------------------------------------------------------
def _lin_equal(a, b):
    return a["n"] == b["n"] and a["err"] == b["err"] and np.array_equal(a["H"], b["H"]) and np.array_equal(a["b"], b["b"])


def test_set_params_drops_what_the_old_setting_shaped(gpu, fold_case):
    from simpleslam_amd import PcrError
    m, s, T = fold_case["map"], fold_case["scan"], cov_ref.fold_poses()[1]
    fresh = {}
    for reg in (R.PLANE, R.FROBENIUS):
        f = VgicpRegister(vgicp_regularization=reg)
        f.setTarget(m)
        P = T.copy()
        f.align(s, P)
        fresh[reg] = (f.linearize(s, T), P)
    h = VgicpRegister()
    h.setTarget(m)
    assert _lin_equal(h.linearize(s, T), fresh[R.PLANE][0])
    for reg in (R.FROBENIUS, R.PLANE):
        h.set_params(vgicp_regularization=reg)
        with pytest.raises(PcrError, match="no target"):      # the kept target went with the setting
            h.linearize(s, T)
        h.setTarget(m)
        assert _lin_equal(h.linearize(s, T), fresh[reg][0]), R.REG_NAMES[reg]
        P = T.copy()
        h.align(s, P)
        assert np.array_equal(P, fresh[reg][1]), R.REG_NAMES[reg]
    with pytest.raises(PcrError, match="vgicp_voxel_mode"):
        h.set_params(vgicp_voxel_mode=3)
    g = GicpRegister()
    g.setTarget(m)
    g.set_params(vgicp_voxel_mode=R.MULTIPLICATIVE)      # no voxels: ignored, the target stays
    g.linearize(s, T)
    g.set_params(vgicp_regularization=R.MIN_EIG)
    with pytest.raises(PcrError):
        g.linearize(s, T)


def test_a_sharded_handle_with_multiplicative_voxels(gpu, fold_case):
    m, s, T = fold_case["map"], fold_case["scan"], cov_ref.fold_poses()[1]
    a = VgicpRegister(vgicp_voxel_mode=R.MULTIPLICATIVE)
    a.setTarget(m)
    b = VgicpRegister(vgicp_voxel_mode=R.MULTIPLICATIVE)
    coll = shard.ThreadCollective(1, timeout=60.0)
    b.set_shard([-1e30] * 3, [1e30] * 3, 2.0)      # one rank, every face open
    b.comm_init_host(coll.fn(0), 0, 1)
    b.setTarget(m)
    la, lb = a.linearize(s, T), b.linearize(s, T)
    assert _lin_equal(la, lb)      # the same kernels over the same voxels
    Pa, Pb = T.copy(), T.copy()
    assert a.align(s, Pa) == b.align(s, Pb)
    dt, da = synth.pose_error(Pa, Pb)      # (the sharded handle runs the host-driven loop)
    assert dt <= 2e-6 and da <= 2e-6
