"""Global relocalisation on the host (no device): the coarse pose of a place and its lattice (pcr_global_reloc_hypotheses) against a numpy
restatement of include/pcr_hip.h, bit for bit, the default parameters, and the arguments refused."""
import ctypes as C
import math

import numpy as np
import pytest

from simpleslam_amd import global_reloc_hypotheses, global_reloc_params, synth
from simpleslam_amd.pcr import GlobalRelocCandidate, PcrError, RelocParams, load_library
from test_reloc_host import _assert_bits, restated


def coarse_restated(kf_pose, shift):
    """kf_pose * Rz(-yaw), yaw = deg2rad<float>(6 * shift) as pcr_sc_query forms it: (float)((double)(6.0f * (float)shift) * M_PI / 180.0);
    column 0 <- c C0 - s C1, column 1 <- s C0 + c C1 with c, s the C library's cos and sin of the float yaw widened to double"""
    six_k = float(np.float32(6.0) * np.float32(shift))
    yaw = float(np.float32(six_k * math.pi / 180.0))
    c, s = math.cos(yaw), math.sin(yaw)
    T = np.asarray(kf_pose, np.float64)
    out = T.copy()
    out[:, 0] = c * T[:, 0] - s * T[:, 1]
    out[:, 1] = s * T[:, 0] + c * T[:, 1]
    return out


def _kf():
    T = synth.perturb(np.eye(4), 11, trans=3.0, rot_deg=25.0)
    T[:3, 3] += [40.7, -13.2, 0.4]
    return T


LOCAL = dict(xy_range=2.0, xy_step=0.5, yaw_range=9.0 * math.pi / 180.0, yaw_step=3.0 * math.pi / 180.0)      # (as the C default: not math.radians)


@pytest.mark.parametrize("shift", [0, 1, 7, 30, 31, 59, 60, 61, -1, -59, 125])
def test_place_lattice_equals_the_restatement(shift):
    T = _kf()
    got = global_reloc_hypotheses(T, shift)
    want, nx, nk = restated(coarse_restated(T, shift), **LOCAL)
    assert (nx, nk) == (4, 3) and got.shape == (567, 4, 4)
    _assert_bits(got, want)
    one = global_reloc_hypotheses(T, shift, xy_range=0.0, yaw_range=0.0)
    _assert_bits(one[0], coarse_restated(T, shift))


def test_the_yaw_is_the_float_deg2rad_of_the_query():
    """shift 7: the float yaw 0.73303829 (not the double 7 * 6 degrees) is what rotates the key frame, to the last bit"""
    T = np.eye(4)
    got = global_reloc_hypotheses(T, 7, xy_range=0.0, yaw_range=0.0)[0]
    yaw_f = float(np.float32(42.0 * math.pi / 180.0))
    assert yaw_f != math.radians(42.0)
    assert got[1, 0] == -math.sin(yaw_f) and got[0, 0] == math.cos(yaw_f)
    # wraps: 60 sectors are a whole turn, up to the float rounding of 360 degrees
    np.testing.assert_allclose(global_reloc_hypotheses(T, 67, xy_range=0.0, yaw_range=0.0)[0], got, atol=1e-6)


def test_default_parameters():
    p = global_reloc_params()
    assert p.struct_size == C.sizeof(p) and p.places == 5 and p.max_dist == np.finfo(np.float64).max
    q = p.local
    assert q.struct_size == C.sizeof(RelocParams)
    assert (q.xy_range, q.xy_step, q.refine_top, q.max_sq, q.score_points) == (2.0, 0.5, 2, 1.0, 4096)
    assert q.yaw_range == pytest.approx(math.radians(9.0)) and q.yaw_step == pytest.approx(math.radians(3.0))
    assert global_reloc_hypotheses(np.eye(4), 0).shape == (9 * 9 * 7, 4, 4)
    o = global_reloc_params(places=3, max_dist=0.3, refine_top=4, xy_range=1.0)
    assert (o.places, o.max_dist, o.local.refine_top, o.local.xy_range) == (3, 0.3, 4, 1.0)


def _hyp_raw(local, cap, kf=True):
    L = load_library()
    dp = C.POINTER(C.c_double)
    c = np.ascontiguousarray(_kf().T).reshape(16)
    out = np.zeros(max(cap, 1) * 16)
    K = C.c_size_t(0)
    rc = L.pcr_global_reloc_hypotheses(c.ctypes.data_as(dp) if kf else None, 3, C.byref(local) if local is not None else None,
                                       out.ctypes.data_as(dp) if cap else None, cap, C.byref(K))
    return rc, L.pcr_last_error(None).decode(), K.value


@pytest.mark.parametrize("bad, words", [
    (dict(xy_step=0.0), "xy_step"),
    (dict(yaw_step=-1.0), "yaw_step"),
    (dict(refine_top=0), "refine_top"),
    (dict(yaw_range=float("nan")), "range"),
    (dict(xy_range=100.0, xy_step=0.01), "PCR_RELOC_MAX_POSES"),
])
def test_bad_local_lattice_is_refused(bad, words):
    p = global_reloc_params(**bad)
    rc, msg, _ = _hyp_raw(p.local, 1 << 20)
    assert rc != 0 and words in msg and msg.startswith("pcr_global_reloc_hypotheses"), (bad, msg)
    with pytest.raises(PcrError, match=words):
        global_reloc_hypotheses(np.eye(4), 0, **bad)
    rc, msg = _global_raw(p, 64)
    assert rc != 0 and "local lattice" in msg and words in msg, (bad, msg)


def test_null_and_small_outputs_are_refused():
    p = global_reloc_params()
    rc, msg, K = _hyp_raw(p.local, 0)
    assert rc != 0 and "567" in msg and K == 567
    rc, msg, _ = _hyp_raw(p.local, 566)
    assert rc != 0 and "566" in msg
    assert _hyp_raw(p.local, 567)[0] == 0
    rc, msg, _ = _hyp_raw(p.local, 567, kf=False)
    assert rc != 0 and "NULL" in msg
    rc, msg, _ = _hyp_raw(None, 567)
    assert rc != 0 and "NULL" in msg
    bad = global_reloc_params().local
    bad.struct_size = 3
    rc, msg, _ = _hyp_raw(bad, 567)
    assert rc != 0 and "struct_size" in msg
    rc, msg = _global_raw(p, 9)
    assert rc != 0 and "places x refine_top = 10" in msg, msg
    rc, msg = _global_raw(p, 10, outputs=False)
    assert rc != 0 and "NULL" in msg, msg


def _global_raw(p, cap, outputs=True):
    """pcr_relocalize_global with no handle: the parameters and outputs are checked first, and reported through pcr_last_error(NULL)"""
    L = load_library()
    dp = C.POINTER(C.c_double)
    pose = np.zeros(16)
    cands = (GlobalRelocCandidate * max(cap, 1))()
    conv, nc, ch = C.c_int(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.pcr_relocalize_global(None, None, None, 0, None, 0, 16, 0, C.byref(p) if p is not None else None,
                                 pose.ctypes.data_as(dp) if outputs else None, C.byref(conv), cands, cap, C.byref(nc), C.byref(ch))
    return rc, L.pcr_last_error(None).decode()


def test_global_parameters_are_refused_with_a_message():
    p = global_reloc_params()
    p.struct_size = 8
    rc, msg = _global_raw(p, 64)
    assert rc != 0 and "struct_size" in msg, msg
    for places in (0, -3):
        rc, msg = _global_raw(global_reloc_params(places=places), 64)
        assert rc != 0 and "places" in msg, msg
    rc, msg = _global_raw(global_reloc_params(max_dist=float("nan")), 64)
    assert rc != 0 and "max_dist" in msg, msg
    rc, msg = _global_raw(None, 64)
    assert rc != 0 and "NULL" in msg, msg
    rc, msg = _global_raw(global_reloc_params(), 64)      # valid parameters: then the missing handle
    assert rc != 0 and "handle is NULL" in msg, msg


def test_python_argument_errors():
    with pytest.raises(AttributeError, match="nonsense"):
        global_reloc_params(nonsense=1)
    with pytest.raises(ValueError, match="4x4"):
        global_reloc_hypotheses(np.eye(3), 0)
    with pytest.raises(TypeError, match="shift"):
        global_reloc_hypotheses(np.eye(4), 1.5)
    with pytest.raises(TypeError, match="shift"):
        global_reloc_hypotheses(np.eye(4), "3")
