"""fast_gicp's regularisation and voxel accumulation settings without a GPU: the algebra of tests/gicp_settings_ref.py, the two pcr_params
fields and their refusal, and the measurements behind every bound the GPU tests use (each figure printed, then held to twice the recorded
constant -- the convention of tests/test_cov_ref.py::test_oracle_against_the_reference)."""
import ctypes as C

import numpy as np
import pytest

import cov_ref
import gicp_settings_ref as R
from simpleslam_amd import pcr

REGS = (R.NONE, R.MIN_EIG, R.NORMALIZED_MIN_EIG, R.PLANE, R.FROBENIUS)


@pytest.fixture(scope="module")
def scatters():
    return {name: R.scatter(pts) for name, pts in cov_ref.clouds().items()}


@pytest.fixture(scope="module")
def fold_case():
    m = cov_ref.fold_map()
    s = cov_ref.fold_scan(m)
    return dict(map=m, scan=s, Sm=R.scatter(m)[0], Ss=R.scatter(s)[0])


# ---- algebra ------------------------------------------------------------------------------------------------------------------------------
def test_plane_is_cov_ref_and_none_is_the_scatter(scatters):
    for name, (S, ref) in scatters.items():
        assert np.array_equal(R.regularize(S, R.PLANE), ref.cov), name
        assert np.array_equal(R.regularize(S, R.NONE), S), name


def test_min_eig_and_frobenius_algebra(scatters):
    for name, (S, _) in scatters.items():
        w = np.linalg.eigvalsh(S)
        got = np.linalg.eigvalsh(R.regularize(S, R.MIN_EIG))
        assert np.abs(got - np.sort(np.maximum(w, 1e-3), axis=1)).max() <= 1e-13 * max(1.0, w.max()), name
        nw = np.linalg.eigvalsh(R.regularize(S, R.NORMALIZED_MIN_EIG))
        assert np.abs(nw[:, 2] - 1.0).max() <= 1e-13 and nw.min() >= 1e-3 * (1 - 1e-12), name
        F = R.regularize(S, R.FROBENIUS)
        assert np.abs(np.linalg.norm(np.linalg.inv(F), axis=(1, 2)) - 1.0).max() <= 1e-9, name      # (condition up to 1e4 in the inverse)


def test_an_exact_plane_gets_1e_3_along_its_normal(scatters):
    S, _ = scatters["plane"]
    M = R.regularize(S, R.MIN_EIG)
    assert np.array_equal(M[:, 2, 2], np.full(len(M), 1e-3)) and (np.abs(M[:, :2, 2]) == 0).all()      # z is the normal, exactly
    assert np.array_equal(M[:, :2, :2].round(12), S[:, :2, :2].round(12))


def test_multiplicative_of_equal_covariances_and_mode_1():
    rng = np.random.default_rng(3)
    p = np.zeros((5, 4), np.float32)
    p[:, :3] = 0.6 + 0.3 * rng.random((5, 3))
    Cm = np.diag([0.5, 0.25, 2.0]) + 0.0625
    f = R.fold(p, np.repeat(Cm[None], 5, 0), 1.0, R.MULTIPLICATIVE)
    assert len(f["n"]) == 1 and f["n"][0] == 5
    assert np.abs(f["cov"][0] - Cm / 5).max() <= 1e-15 and np.abs(f["mean"][0] - p[:, :3].astype(np.float64).mean(0)).max() <= 1e-15
    covs = rng.random((5, 3, 3))
    covs = covs @ covs.transpose(0, 2, 1) + np.eye(3)
    a, b = R.fold(p, covs, 1.0, R.ADDITIVE), R.fold(p, covs, 1.0, R.ADDITIVE_WEIGHTED)
    assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["cov"], b["cov"])


# ---- parameters ---------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_struct_size():
    p = pcr.default_params()
    assert p.vgicp_regularization == 3 == pcr.REG_PLANE and p.vgicp_voxel_mode == 0 == pcr.VOXEL_ADDITIVE
    assert p.struct_size == C.sizeof(pcr.PcrParams)
    assert [f for f, _ in pcr.PcrParams._fields_][-3:] == ["gicp_max_corr_dist", "vgicp_regularization", "vgicp_voxel_mode"]


@pytest.mark.parametrize("method", ["vgicp", "gicp"])
@pytest.mark.parametrize("field,value", [("vgicp_regularization", 5), ("vgicp_regularization", -1), ("vgicp_voxel_mode", 3), ("vgicp_voxel_mode", -1)])
def test_a_value_out_of_range_is_refused_before_any_device_is_touched(method, field, value):
    """(on a machine without a GPU the message names the field, not the missing device)"""
    L = pcr.load_library()
    p = pcr.default_params(**{field: value})
    assert not L.pcr_create(method.encode(), C.byref(p))
    assert field in L.pcr_last_error(None).decode()


def test_the_voxel_entry_point_is_exported():
    L = pcr.load_library()
    assert "pcr_vgicp_voxels" in pcr.ABI_SYMBOLS and hasattr(L, "pcr_vgicp_voxels")
    assert callable(pcr.VgicpRegister.voxels)


# ---- the measurements behind the GPU bounds -----------------------------------------------------------------------------------------------------
def test_regularisations_against_their_alternative_evaluation(scatters):
    worst = {m: 0.0 for m in R.NEW_REGS}
    for name, (S, ref) in scatters.items():
        keep = ~ref.ambiguous
        assert ref.ambiguous.mean() < 0.01, name
        row = {}
        for m in R.NEW_REGS:
            alt = R.scatter_f64(cov_ref.clouds()[name], ref.idx) if m == R.NONE else R.regularize_alt(S, m)
            row[m] = float(R.rel_diff(alt, R.regularize(S, m))[keep].max())
            worst[m] = max(worst[m], row[m])
        print(name, {R.REG_NAMES[m]: f"{v:.2e}" for m, v in row.items()})
    print("worst", {R.REG_NAMES[m]: f"{v:.2e}" for m, v in worst.items()}, "recorded", R.REF_REG_MAX)
    for m in R.NEW_REGS:
        assert worst[m] <= 2 * R.REF_REG_MAX[m], (R.REG_NAMES[m], worst[m])


def test_the_clouds_that_none_is_inverted_on_are_well_conditioned(scatters, fold_case):
    for name in R.WELL_CONDITIONED:
        assert R.conditioning(scatters[name][0]).min() >= R.COND_FLOOR, name      # every query, none left out
    assert R.conditioning(fold_case["Sm"]).min() >= R.COND_FLOOR and R.conditioning(fold_case["Ss"]).min() >= R.COND_FLOOR


@pytest.mark.parametrize("reg", REGS)
def test_fold_against_its_alternative_evaluation(fold_case, reg):
    Cm, Cma = R.regularize(fold_case["Sm"], reg), R.regularize_alt(fold_case["Sm"], reg)
    for mode in (R.ADDITIVE, R.MULTIPLICATIVE):
        worst = [0.0, 0.0]
        for res in (1.0, 2.0):
            a, b = R.fold(fold_case["map"], Cm, res, mode), R.fold(fold_case["map"], Cma, res, mode, alt=True)
            assert np.array_equal(a["ijk"], b["ijk"]) and a["n"].sum() == len(fold_case["map"])
            worst = [max(worst[0], float(R.rel_diff(b["mean"], a["mean"]).max())), max(worst[1], float(R.rel_diff(b["cov"], a["cov"]).max()))]
        print(R.REG_NAMES[reg], R.MODE_NAMES[mode], f"mean {worst[0]:.2e} cov {worst[1]:.2e}", "recorded", R.REF_FOLD_MAX[(reg, mode)])
        assert worst[0] <= 2 * R.REF_FOLD_MAX[(reg, mode)][0] and worst[1] <= 2 * R.REF_FOLD_MAX[(reg, mode)][1]


@pytest.mark.parametrize("reg", REGS)
def test_linearisation_against_its_alternative_evaluation(fold_case, reg):
    m, s, T = fold_case["map"], fold_case["scan"], cov_ref.fold_poses()[1]
    Cm, Cs = R.regularize(fold_case["Sm"], reg), R.regularize(fold_case["Ss"], reg)
    Cma, Csa = R.regularize_alt(fold_case["Sm"], reg), R.regularize_alt(fold_case["Ss"], reg)
    for mode in (R.ADDITIVE, R.MULTIPLICATIVE):
        a = R.linearize(s, T, Cs, R.fold(m, Cm, 1.0, mode), 1.0)
        b = R.linearize(s, T, Csa, R.fold(m, Cma, 1.0, mode, alt=True), 1.0)
        assert a["n"] == b["n"] == 307
        d = cov_ref.lin_diff(b, a)
        print(R.REG_NAMES[reg], R.MODE_NAMES[mode], "H %.2e b %.2e err %.2e" % d, "recorded", R.REF_LIN_MAX[(reg, mode)])
        assert all(x <= 2 * y for x, y in zip(d, R.REF_LIN_MAX[(reg, mode)])), d
        if reg == R.PLANE and mode == R.ADDITIVE:      # the transcription this one generalises
            c = cov_ref.linearize(s, m, T, Cs, Cm, 1.0)
            assert max(cov_ref.lin_diff(a, c)) <= 1e-13


def test_the_vectorised_pass_of_the_alignment_is_the_linearisation(fold_case):
    m, s, T = fold_case["map"], fold_case["scan"], cov_ref.fold_poses()[1]
    Cm, Cs = R.regularize(fold_case["Sm"], R.MIN_EIG), R.regularize(fold_case["Ss"], R.MIN_EIG)
    vox = R.fold(m, Cm, 1.0, R.MULTIPLICATIVE)
    a, b = R.linearize(s, T, Cs, vox, 1.0), R._lin_state(s, T, Cs, vox, 1.0)[0]
    assert a["n"] == b["n"] and max(cov_ref.lin_diff(b, a)) <= 10 * R.LIN_SUM_FLOOR
