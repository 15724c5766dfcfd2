"""The plain GICP reference (tests/gicp_ref.py) checked on its own, and the parts of the gicp method that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import gicp_ref
from simpleslam_amd import synth
from simpleslam_amd.pcr import ABI_SYMBOLS, LIB_PATH, default_params, load_library, make_register


def _twist_pose(k, eps, T):
    """exp(eps e_k) T, the twist [rotation; translation] applied from the left as the optimiser applies its steps"""
    xi = np.zeros(6)
    xi[(k + 3) % 6] = eps                      # synth.se3_exp takes [rho; omega]
    return synth.se3_exp(xi) @ T


def test_gradient_of_the_error_is_twice_b():
    """With the correspondences and matrices frozen, err(exp(eps e_k) T) has the derivative 2 b_k at eps = 0 (e' = J e_k).  Central differences with
    step h leave a truncation error h^2 / 6 |f'''| and a rounding error about eps_64 |f| / h.  Along a translation axis f is a quadratic and the
    truncation term vanishes; along a rotation axis f''' is made of terms (w x p)^T M (w x (w x p)) against f' = 2 e^T M (w x p): larger by up to
    |p| / |e|, at most 120 m of range over the 1 cm noise floor of the residuals, i.e. |f''' / f'| <= 1.2e4.  With h = 1e-4 that is a relative
    2e-5; the rounding term, eps_64 err / (h |2 b|) with err / |2 b| < 1e3 here (asserted), stays below 3e-9.  rtol = 3e-5 of the largest |2 b_k|."""
    w = gicp_ref.world_small_case()
    r = gicp_ref.linearize(w["scan"], w["map"], w["init"], w["C_A"], w["C_B"])
    h = 1e-4
    scale = np.abs(2 * r["b"]).max()
    assert r["err"] / scale < 1e3
    for k in range(6):
        fp = gicp_ref.error(w["scan"], w["map"], _twist_pose(k, h, w["init"]), r["corr"], r["M"])
        fm = gicp_ref.error(w["scan"], w["map"], _twist_pose(k, -h, w["init"]), r["corr"], r["M"])
        fd = (fp - fm) / (2 * h)
        print(k, fd, 2 * r["b"][k])
        assert abs(fd - 2 * r["b"][k]) <= 3e-5 * scale, (k, fd, 2 * r["b"][k])
    # ... and at the linearisation point itself error() is linearize()'s error
    assert abs(gicp_ref.error(w["scan"], w["map"], w["init"], r["corr"], r["M"]) - r["err"]) <= 1e-12 * r["err"]


def test_alignment_converges_within_5_mm_of_the_truth():
    w = gicp_ref.world_small_case()
    a = gicp_ref.world_small_alignment()
    dt, dr = synth.pose_error(a["pose"], w["truth"])
    print(a["converged"], a["outer"], a["passes"], dt, dr)
    assert a["converged"] and 0 < a["outer"] < 64
    assert dt <= 5e-3, dt


def test_ambiguous_share_is_below_one_percent():
    w = gicp_ref.world_small_case()
    for pose in (w["init"], gicp_ref.world_small_alignment()["pose"]):
        _, _, amb = gicp_ref.correspondences(w["scan"], w["map"], pose)
        print(int(amb.sum()), "of", amb.size)
        assert amb.sum() < 0.01 * amb.size


def test_gate_and_degenerate_inputs():
    dst = np.zeros((5, 4), np.float32)
    dst[:, 0] = [0.0, 1.0, np.nan, 3.0, np.inf]                 # rows 2 and 4 are not indexed and do not renumber the others
    src = np.zeros((6, 4), np.float32)
    src[:, 0] = [0.1, 0.9, 2.9, 0.5, np.nan, 10.0]
    src[5, 1] = np.inf
    I = np.eye(4)
    corr, d2, amb = gicp_ref.correspondences(src, dst, I)
    assert corr.tolist() == [0, 1, 3, 0, -1, -1]                # 0.5: an exact tie between rows 0 and 1 -> the lower row
    assert not amb.any()
    assert d2[3] == np.float32(0.25) and np.isinf(d2[4:]).all()
    # the gate is strict and formed in float: 0.5 m admits d2 < 0.25 only
    corr, d2, _ = gicp_ref.correspondences(src, dst, I, 0.5)
    assert corr.tolist() == [0, 1, 3, -1, -1, -1] and np.isinf(d2[3])
    assert gicp_ref.thr2_of(gicp_ref.FLT_MAX) == np.inf
    assert gicp_ref.thr2_of(0.3) == np.float32(0.3) * np.float32(0.3)
    corr, _, _ = gicp_ref.correspondences(src, np.zeros((0, 4), np.float32), I)
    assert (corr == -1).all()
    # a linearisation without any correspondence is all zeros
    C3 = np.tile(np.eye(3), (6, 1, 1))
    r = gicp_ref.linearize(src, dst, I, C3, C3[:5], 1e-3)
    assert r["n"] == 0 and not r["H"].any() and not r["b"].any() and r["err"] == 0.0


def test_exact_ties_go_to_the_lower_index():
    src, dst, want = gicp_ref.lattice_case()
    corr, d2, amb = gicp_ref.correspondences(src, dst, np.eye(4))
    np.testing.assert_array_equal(corr, want)                   # (x is the slowest axis of the rows: the lower x is the lower row)
    assert (d2 == np.float32(0.25)).all() and not amb.any()
    rev = dst[::-1].copy()                                     # rows reversed: the other end of every edge is now the lower row
    corr, _, _ = gicp_ref.correspondences(src, rev, np.eye(4))
    np.testing.assert_array_equal(corr, 215 - (want + 36))


def test_reference_against_its_alternative_evaluation():
    """The figures behind gicp_ref.REF_*_MAX (printed); the alternative is held to twice what was measured."""
    w = gicp_ref.world_small_case()
    for name, pose, gate in (("perturbed", w["init"], gicp_ref.FLT_MAX), ("truth", w["truth"], gicp_ref.FLT_MAX), ("gated", w["init"], 0.3)):
        r = gicp_ref.linearize(w["scan"], w["map"], pose, w["C_A"], w["C_B"], gate)
        assert 0 < r["n"] <= 8192 and (gate > 1 or r["n"] < 8192)
        M4, ML = gicp_ref.alt_mahalanobis(w["C_A"], w["C_B"], pose, r["corr"])
        H, b, e = gicp_ref.alt_sums(w["scan"], w["map"], pose, r["corr"], r["M"])
        dH, db, de = gicp_ref.sums_diff(dict(H=H, b=b, err=e), r)
        d4, dl = gicp_ref.m_diff(M4, r["M"]), gicp_ref.m_diff(ML, r["M"])
        print(name, "M4 %.3g ML %.3g H %.3g b %.3g err %.3g" % (d4, dl, dH, db, de))
        assert max(d4, dl) <= 2 * gicp_ref.REF_M_MAX
        assert dH <= 2 * gicp_ref.REF_H_MAX and db <= 2 * gicp_ref.REF_B_MAX and de <= 2 * gicp_ref.REF_ERR_MAX
    assert gicp_ref.DEVICE_M_BOUND == 10 * gicp_ref.REF_M_MAX and gicp_ref.DEVICE_ERR_BOUND == 10 * gicp_ref.REF_ERR_MAX


# ---- the method's host side: these fail without the feature ---------------------------------------------------------------------------
def test_factory_knows_gicp():
    import torch
    from simpleslam_amd import GicpRegister, PcrError
    if torch.cuda.is_available():
        reg = make_register("gicp")
        assert isinstance(reg, GicpRegister) and reg.method == "gicp"
    else:
        with pytest.raises(PcrError, match="HIP device"):       # known to the factory: it gets as far as asking for a device
            make_register("gicp")


def test_default_gate_is_flt_max():
    p = default_params()
    assert p.gicp_max_corr_dist == float(np.float32(3.4028234663852886e38))
    assert p.struct_size == C.sizeof(p)


def test_create_without_gpu_names_the_device_not_the_method():
    import torch
    lib = load_library()
    h = lib.pcr_create(b"gicp", None)
    if torch.cuda.is_available():
        assert h
        lib.pcr_destroy(h)
    else:
        assert not h
        msg = lib.pcr_last_error(None)
        assert b"HIP device" in msg and b"is not exist" not in msg


def test_gicp_linearize_is_exported():
    assert "pcr_gicp_linearize" in ABI_SYMBOLS
    assert os.path.exists(LIB_PATH)
    assert hasattr(C.CDLL(LIB_PATH), "pcr_gicp_linearize")
