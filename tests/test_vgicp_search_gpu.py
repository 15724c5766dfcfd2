"""fast_gicp's neighbour search methods on the device (pcr_params.vgicp_search: DIRECT7, DIRECT27; DIRECT1 where it says so) against
tests/vgicp_search_ref.py: the pair sets exactly (pcr_vgicp_correspondences), H, b and the error within ten times the reference's own figure (never
below n_pairs * 2^-53), whole alignments, repeatability, region-only targets and the life cycle of the parameter.  Each test prints what it observed."""
import ctypes as C

import numpy as np
import pytest

import cov_ref
import gicp_settings_ref as R
import vgicp_search_ref as V
from simpleslam_amd import GicpRegister, PcrError, VgicpRegister, pcr, shard, synth
from simpleslam_amd.pcr import make_register

pytestmark = pytest.mark.gpu

WIDE = (V.DIRECT7, V.DIRECT27)


def _pair_set(d):
    return np.concatenate([np.asarray(d["rows"] if "rows" in d else d["row"], np.int64)[:, None], np.asarray(d["ijk"], np.int64).reshape(-1, 3)], axis=1)


def _search_of(h):
    p = pcr.PcrParams()
    assert h._lib.pcr_get_params(h._h, C.byref(p)) == 0
    return p.vgicp_search


def _lin_equal(a, b):
    return a["n"] == b["n"] and a["err"] == b["err"] and np.array_equal(a["H"], b["H"]) and np.array_equal(a["b"], b["b"])


@pytest.fixture(scope="module")
def case():
    return V.block_case()


# ---------------------------------------------------------------------------
# 1. / 2. pairs and sums of one linearisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("search", WIDE)
@pytest.mark.parametrize("reg,mode", V.SETTINGS)
def test_pairs_and_sums_of_a_linearisation(gpu, case, reg, mode, search):
    vox, Cs = V.block_voxels(reg, mode)
    h = VgicpRegister(vgicp_regularization=reg, vgicp_voxel_mode=mode, vgicp_search=search)
    h.setTarget(case["map"])
    for T in cov_ref.fold_poses():
        want, got = V.linearize(case["scan"], T, Cs, vox, 1.0, search), h.linearize(case["scan"], T)
        corr = h.correspondences()
        assert got["n"] == want["n"] == len(corr["row"])
        assert np.array_equal(_pair_set(corr), _pair_set(want))      # the same pairs in the same order: by row, a row's in table order
        bound = V.device_lin_bound(reg, mode, search, want["n"])
        d = cov_ref.lin_diff(got, want)
        print(f"{R.REG_NAMES[reg]} {R.MODE_NAMES[mode]} {V.NAMES[search]}: pairs {got['n']}, H {d[0]:.3e} b {d[1]:.3e} err {d[2]:.3e} (bounds {bound[0]:.1e} {bound[1]:.1e} {bound[2]:.1e})")
        assert all(x <= y for x, y in zip(d, bound)), d


# ---------------------------------------------------------------------------
# 3. other resolutions: voxels of 1 to 1 000 points, a box that is no cube
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("search", WIDE)
@pytest.mark.parametrize("res", [0.5, 2.0])
def test_pairs_at_other_resolutions(gpu, search, res):
    m = cov_ref.fold_map()
    s = cov_ref.fold_scan(m)
    vox = R.fold(m, np.tile(np.eye(3), (len(m), 1, 1)), res, R.ADDITIVE)      # (the pairs depend on the voxels' coordinates only)
    h = VgicpRegister(vgicp_resolution=res, vgicp_search=search)
    h.setTarget(m)
    for k, T in enumerate(cov_ref.fold_poses()):
        if k:
            assert V.face_distance(s, T, res) > 1e-9
        rows, v = V.pairs(s, T, vox, res, search)
        got = h.linearize(s, T)
        corr = h.correspondences()
        print(f"res {res} {V.NAMES[search]} pose {k}: pairs {got['n']} (reference {len(rows)})")
        assert got["n"] == len(rows)
        assert np.array_equal(_pair_set(corr), _pair_set(dict(rows=rows, ijk=vox["ijk"][v])))


# ---------------------------------------------------------------------------
# 4. / 5. whole alignments
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def align_case(case):
    vox, Cs = V.block_voxels(R.PLANE, R.ADDITIVE)
    init = synth.perturb(np.eye(4), 11, trans=0.3, rot_deg=2.0)
    return dict(vox=vox, Cs=Cs, init=init, want={s: V.vgicp_align(case["scan"], vox, init, Cs, search=s) for s in V.SEARCHES})


@pytest.mark.parametrize("search", WIDE)
def test_alignment_against_the_reference(gpu, case, align_case, search):
    want = align_case["want"][search]
    h = VgicpRegister(vgicp_search=search)
    T = align_case["init"].copy()
    conv = h.scan2Map(case["scan"], case["map"], T)
    dt, da = synth.pose_error(T, want["pose"])
    print(f"{V.NAMES[search]}: converged {conv} iterations {h.stats()['iterations']} (reference {want['converged']} {want['outer']}), pose off by {dt:.2e} m {da:.2e} rad")
    assert conv == want["converged"] and h.stats()["iterations"] == want["outer"]
    assert dt <= 1e-4 and da <= 1e-4      # the project's parity criterion
    if search == V.DIRECT7:      # the setting has an effect
        h1 = VgicpRegister()
        T1 = align_case["init"].copy()
        h1.scan2Map(case["scan"], case["map"], T1)
        d1 = synth.pose_error(T1, align_case["want"][V.DIRECT1]["pose"])
        assert d1[0] <= 1e-4 and d1[1] <= 1e-4
        assert not np.array_equal(T, T1) and not np.array_equal(want["pose"], align_case["want"][V.DIRECT1]["pose"])


@pytest.mark.parametrize("search", WIDE)
def test_host_loop_and_repeated_call_give_the_same_bits(gpu, case, align_case, search):
    poses, flags = [], []
    for host in (0, 1, 0):
        h = VgicpRegister(vgicp_search=search, host_optimiser=host)
        h.setTarget(case["map"])
        for _ in range(2):
            T = align_case["init"].copy()
            flags.append((h.align(case["scan"], T), h.stats()["iterations"]))
            poses.append(T)
    assert all(np.array_equal(p, poses[0]) for p in poses) and len(set(flags)) == 1, flags
    # ... and so does a linearisation
    h = VgicpRegister(vgicp_search=search)
    h.setTarget(case["map"])
    a = h.linearize(case["scan"], align_case["init"])
    assert _lin_equal(a, h.linearize(case["scan"], align_case["init"]))


# ---------------------------------------------------------------------------
# 6. DIRECT1 is the code that ran before
# ---------------------------------------------------------------------------
def test_direct1_given_explicitly_is_the_default(gpu, case, align_case):
    a, b = VgicpRegister(), VgicpRegister(vgicp_search=V.DIRECT1)
    assert _search_of(a) == V.DIRECT1
    for h in (a, b):
        h.setTarget(case["map"])
    for T in cov_ref.fold_poses():
        la, lb = a.linearize(case["scan"], T), b.linearize(case["scan"], T)
        assert _lin_equal(la, lb)
        ca, cb = a.correspondences(), b.correspondences()
        assert np.array_equal(_pair_set(ca), _pair_set(cb)) and len(ca["row"]) == la["n"]
    vox, Cs = V.block_voxels(R.PLANE, R.ADDITIVE)
    want = V.linearize(case["scan"], cov_ref.fold_poses()[1], Cs, vox, 1.0, V.DIRECT1)
    assert np.array_equal(_pair_set(a.correspondences()), _pair_set(want))
    Ta, Tb = align_case["init"].copy(), align_case["init"].copy()
    assert a.scan2Map(case["scan"], case["map"], Ta) == b.scan2Map(case["scan"], case["map"], Tb)
    assert np.array_equal(Ta, Tb) and a.stats()["iterations"] == b.stats()["iterations"]


# ---------------------------------------------------------------------------
# 7. region-only targets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("search", WIDE)
def test_region_only_target_matches_the_whole_target(gpu, search):
    world, m = synth.make_map(400_000, seed=77)
    scan, T = synth.make_scan(world, 1, seed=77)
    full, reg = VgicpRegister(vgicp_search=search, full_target=1), VgicpRegister(vgicp_search=search)
    region_index, repeats = 0, 0
    for k, off in enumerate([0.2, -0.3, 0.1]):
        T0 = T.copy()
        T0[:3, 3] += np.array([off, -0.5 * off, 0.03 * off])
        pf = T0.copy(); cf = full.scan2Map(scan, m, pf)
        p = T0.copy(); c = reg.scan2Map(scan, m, p)
        assert c == cf, (k, off)
        np.testing.assert_array_equal(p, pf)
        assert reg.stats()["iterations"] == full.stats()["iterations"], (k, off)
        region_index += reg.stats()["region_index"]
        repeats += reg.stats()["region_repeats"]
    print(f"{V.NAMES[search]}: region_index {region_index} of 3 calls, repeats on the whole target {repeats}")
    assert region_index >= 1
    assert full.stats()["region_index"] == 0


# ---------------------------------------------------------------------------
# 8. life cycle
# ---------------------------------------------------------------------------
def _same_records(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ijk", "n", "mean", "cov"))


def test_set_params_keeps_the_target(gpu, case, align_case):
    s, T = case["scan"], cov_ref.fold_poses()[1]
    fresh = {}
    for search in (V.DIRECT1, V.DIRECT27):
        f = VgicpRegister(vgicp_search=search)
        f.setTarget(case["map"])
        P = align_case["init"].copy()
        f.align(s, P)
        fresh[search] = (f.linearize(s, T), P, f.correspondences())
    h = VgicpRegister()
    h.setTarget(case["map"])
    vox = h.voxels()
    for search in (V.DIRECT1, V.DIRECT27, V.DIRECT1):
        h.set_params(vgicp_search=search)
        assert _lin_equal(h.linearize(s, T), fresh[search][0]), V.NAMES[search]      # no setTarget in between: the prepared target stayed
        assert np.array_equal(_pair_set(h.correspondences()), _pair_set(fresh[search][2]))
        P = align_case["init"].copy()
        h.align(s, P)
        assert np.array_equal(P, fresh[search][1]), V.NAMES[search]
        assert _same_records(h.voxels(), vox)
    assert fresh[V.DIRECT27][0]["n"] > fresh[V.DIRECT1][0]["n"]


@pytest.mark.parametrize("value", [3, 4, -1])
def test_values_that_are_not_served_are_refused(gpu, value):
    with pytest.raises(PcrError, match="vgicp_search"):
        VgicpRegister(vgicp_search=value)
    with pytest.raises(PcrError, match="vgicp_search"):
        make_register("vgicp", vgicp_search=value)
    h = make_register("vgicp", vgicp_search=V.DIRECT7)
    with pytest.raises(PcrError, match="vgicp_search"):
        h.set_params(vgicp_search=value)
    assert _search_of(h) == V.DIRECT7


def test_correspondences_need_a_linearisation(gpu, case):
    h = VgicpRegister(vgicp_search=V.DIRECT7)
    h.setTarget(case["map"])
    with pytest.raises(PcrError, match="pcr_vgicp_linearize first"):
        h.correspondences()
    h.linearize(case["scan"], np.eye(4))
    assert len(h.correspondences()["row"]) > 0
    T = np.eye(4)
    h.align(case["scan"], T)      # the buffers now hold the alignment's last pass
    with pytest.raises(PcrError, match="pcr_vgicp_linearize first"):
        h.correspondences()


def test_a_sharded_handle_refuses_the_wide_neighbourhoods(gpu, case):
    # the setting first, then the tile
    a = VgicpRegister(vgicp_search=V.DIRECT7)
    with pytest.raises(PcrError, match="vgicp_search"):
        a.set_shard([-1e30] * 3, [1e30] * 3, 2.0)
    coll = shard.ThreadCollective(1, timeout=60.0)
    with pytest.raises(PcrError, match="vgicp_search"):
        a.comm_init_host(coll.fn(0), 0, 1)
    # the tile first, then the setting
    b = VgicpRegister()
    b.set_shard([-1e30] * 3, [1e30] * 3, 2.0)
    for search in WIDE:
        with pytest.raises(PcrError, match="vgicp_search"):
            b.set_params(vgicp_search=search)
    assert _search_of(b) == V.DIRECT1
    b.set_params(vgicp_search=V.DIRECT1)
    b.setTarget(case["map"])
    c = VgicpRegister()
    c.setTarget(case["map"])
    T = cov_ref.fold_poses()[1]
    assert _lin_equal(b.linearize(case["scan"], T), c.linearize(case["scan"], T))


def test_a_gicp_handle_ignores_the_setting(gpu, case):
    T = cov_ref.fold_poses()[1]
    out = []
    for search in (V.DIRECT1, V.DIRECT27):
        g = GicpRegister(vgicp_search=search)
        g.setTarget(case["map"])
        lin = g.linearize(case["scan"], T)
        P = T.copy()
        conv = g.align(case["scan"], P)
        out.append((lin, P, conv))
    assert _lin_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    g.set_params(vgicp_search=V.DIRECT7)      # accepted, the target stays
    assert _lin_equal(g.linearize(case["scan"], T), out[0][0])
