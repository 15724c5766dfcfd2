"""pcr::t2se3 and pcr::se3_exp of csrc/small_math.h, compiled for the host (lib/small_math_check), against a numpy longdouble restatement.

The inputs: every heading case's rotation (tests/heading_cases.py: the quaternion route and all three indices of the other one), scaled by
1 + 1e-6 and sheared by 1e-7 because what t2se3 is handed is never orthonormal; twists with |omega| of 0, 1e-7, 1e-6 (the `t < 1e-6`
switch), 1e-3, 1 and pi along the axes and askew.

The bounds are four times what the oracle's C copies (oracle.t2se3, oracle.se3_exp) deviate from the same restatement on the same inputs
-- measured by this file (the test prints the figures) and recorded in ORACLE_DEV below."""
import os
import subprocess

import numpy as np
import pytest

import heading_cases as H
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "small_math_check")
L = np.longdouble
OMEGAS = [0.0, 1e-7, 1e-6, 1e-3, 1.0, float(np.pi)]
# Largest absolute entry difference of the oracle's C copy from the longdouble restatement, measured on the inputs below (x86-64, glibc).
# se3_exp per |omega|: below the switch the result is exact (zero); at 1e-6 the double code forms 1 - cos(t), which cancels to a relative
# 1e-4, and V's skew term (1 - cos t) / t carries that into the translation, where the restatement's 64 bits keep it: 1.3e-11.  The header
# measured the same figures as the oracle to the last digit (the same operations in the same order).
ORACLE_DEV = {"t2se3": 4.993e-16, "exp": {0.0: 0.0, 1e-7: 0.0, 1e-6: 1.289e-11, 1e-3: 1.740e-15, 1.0: 1.106e-16, float(np.pi): 4.185e-16}}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def t2se3_ld(T):
    """trans::T2SE3: Quaternion(R).normalized().toRotationMatrix(); the route is chosen on the double entries as the code chooses it"""
    T = np.asarray(T, np.float64)
    M = T[:3, :3].astype(L)
    q = np.zeros(4, L)      # x y z w
    route = H.t2se3_route(T[:3, :3])
    if route == "q":
        t = np.sqrt(M[0, 0] + M[1, 1] + M[2, 2] + L(1))
        q[3] = t / 2
        q[0], q[1], q[2] = (M[2, 1] - M[1, 2]) / (2 * t), (M[0, 2] - M[2, 0]) / (2 * t), (M[1, 0] - M[0, 1]) / (2 * t)
    else:
        i = route
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(M[i, i] - M[j, j] - M[k, k] + L(1))
        q[i] = t / 2
        q[3] = (M[k, j] - M[j, k]) / (2 * t)
        q[j] = (M[j, i] + M[i, j]) / (2 * t)
        q[k] = (M[k, i] + M[i, k]) / (2 * t)
    x, y, z, w = q / np.sqrt((q * q).sum())
    out = T.astype(L)
    out[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return out


def se3_exp_ld(k):
    """manifolds::exp: the `t < 1e-6` switch on the double norm as the code forms it, everything else in longdouble"""
    k = np.asarray(k, np.float64)
    w64 = k[3:]
    out = np.eye(4, dtype=L)
    if np.sqrt(w64[0] * w64[0] + w64[1] * w64[1] + w64[2] * w64[2]) < 1e-6:
        out[:3, 3] = k[:3]
        return out
    rho, w = k[:3].astype(L), k[3:].astype(L)
    t = np.sqrt((w * w).sum())
    a = w / t
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], L)
    aa = np.outer(a, a)
    I = np.eye(3, dtype=L)
    ct, st = np.cos(t), np.sin(t)
    out[:3, :3] = ct * I + (1 - ct) * aa + st * K
    V = st / t * I + (1 - st / t) * aa + (1 - ct) / t * K
    out[:3, 3] = V @ rho
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
def poses():
    shear = np.eye(3)
    shear[0, 1] = 1e-7
    out = []
    for name in H.NAMES:
        for T in (H.case(name)["truth"], H.case(name)["init"]):
            P = np.array(T)
            P[:3, :3] = (1 + 1e-6) * (P[:3, :3] @ shear)
            out.append(P)
    return out


def twists():
    rng = np.random.default_rng(20)
    dirs = [np.eye(3)[i] for i in range(3)] + [-np.eye(3)[1]] + [d / np.linalg.norm(d) for d in rng.normal(size=(4, 3))]
    out = []
    for om in OMEGAS:
        for d in dirs:
            out.append((om, np.concatenate([rng.uniform(-0.3, 0.3, 3), om * d])))
    return out


def run_header(lines):
    assert os.path.exists(EXE), "lib/small_math_check has not been built"
    out = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.strip().splitlines()
    assert len(rows) == len(lines)
    return [np.array([float(v) for v in r.split()[1:]]).reshape(4, 4) for r in rows]


def _dev(got, want):
    return float(np.abs(np.asarray(got, L) - want).max())


def test_inputs_reach_every_route():
    routes = [H.t2se3_route(P[:3, :3]) for P in poses()]
    assert {0, 1, 2, "q"} == set(routes)
    assert all(routes.count(r) >= 2 for r in (0, 1, 2))
    for P in poses():      # not orthonormal, as promised
        assert np.abs(P[:3, :3].T @ P[:3, :3] - np.eye(3)).max() > 5e-8


def test_t2se3_header_matches_the_restatement():
    ps = poses()
    got = run_header(["t2se3 " + " ".join("%.17g" % v for v in P.ravel()) for P in ps])
    want = [t2se3_ld(P) for P in ps]
    dev_oracle = max(_dev(oracle.t2se3(P), w) for P, w in zip(ps, want))
    dev_header = max(_dev(g, w) for g, w in zip(got, want))
    by_route = {r: max(_dev(g, w) for P, g, w in zip(ps, got, want) if H.t2se3_route(P[:3, :3]) == r) for r in (0, 1, 2, "q")}
    print(f"t2se3: oracle {dev_oracle:.3e}, header {dev_header:.3e} from the longdouble restatement; header by route {by_route}")
    for g, w in zip(got, want):      # the result is a rotation, and the translation is untouched
        np.testing.assert_array_equal(g[:, 3], np.asarray(w[:, 3], np.float64))
        assert np.abs(g[:3, :3].T @ g[:3, :3] - np.eye(3)).max() < 1e-14
    assert dev_oracle <= 2 * ORACLE_DEV["t2se3"]      # the recorded figure is still the oracle's (another C library may move a last bit)
    assert dev_header <= 4 * ORACLE_DEV["t2se3"], dev_header


@pytest.mark.parametrize("om", OMEGAS)
def test_se3_exp_header_matches_the_restatement(om):
    ks = [k for o, k in twists() if o == om]
    got = run_header(["exp " + " ".join("%.17g" % v for v in k) for k in ks])
    want = [se3_exp_ld(k) for k in ks]
    dev_oracle = max(_dev(oracle.se3_exp(k), w) for k, w in zip(ks, want))
    dev_header = max(_dev(g, w) for g, w in zip(got, want))
    print(f"se3_exp |omega| = {om:g}: oracle {dev_oracle:.3e}, header {dev_header:.3e} from the longdouble restatement")
    small = [np.sqrt(k[3] * k[3] + k[4] * k[4] + k[5] * k[5]) < 1e-6 for k in ks]
    if om <= 1e-7:
        assert all(small)
    if om >= 1e-3:
        assert not any(small)
    for g, s, k in zip(got, small, ks):      # below the switch: the identity rotation and rho itself
        if s:
            np.testing.assert_array_equal(g, np.block([[np.eye(3), k[:3, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))
    assert dev_oracle <= 2 * ORACLE_DEV["exp"][om]
    assert dev_header <= 4 * ORACLE_DEV["exp"][om], dev_header
