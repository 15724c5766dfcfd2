"""The robust kernels of pcr_graph against their numpy restatement, without a GPU: rho and w of each kind, w as the derivative
of rho, continuity at the branch point, a host graph's chi2 and readings on ring12_false, and -- in the restatement alone -- that the ring
scenes tell a robust optimiser from plain least squares before anything runs on a device."""
import numpy as np
import pytest

import graph_ref as gr
import graph_robust_ref as rr
import graph_robust_scenes as rs
from simpleslam_amd.pcr import GRAPH_HOST, graph_robust_rho_w

EPS = np.finfo(np.float64).eps
ROBUST = ("huber", "geman_mcclure", "tukey")
DELTAS = (0.1, 1.0, 7.5)


def _samples(d):
    rng = np.random.default_rng(61)
    edge = [0.0, d * (1 - 2.0 ** -52), d, d * (1 + 2.0 ** -52), 1e-300, 1e300]
    return edge + list(d * 10.0 ** rng.uniform(-6, 6, size=40))


@pytest.mark.parametrize("kind", ("none",) + ROBUST)
def test_rho_w_equals_the_restatement(kind):
    """Huber, Geman-McClure and every w are the same expressions on both sides and must agree to one rounding of the last operation (the
    library is compiled without contraction, numpy rounds every operation).  Tukey's rho is evaluated differently: the table's
    d/3 (1 - (1 - s/d)^3) here, s ((1 - q) + q^2 / 3) in the library; the table's form loses up to 3 ulp of ONE, i.e. of d/3, in the
    subtraction, so the two may differ by 4 eps d/3 whatever s is, plus 4 eps of rho itself."""
    for delta in DELTAS:
        d = delta * delta
        for s in _samples(d):
            rho, w = graph_robust_rho_w(kind, delta, s)
            rho0, w0 = rr.rho_w(rr.KINDS[kind], delta, s)
            assert np.isfinite(rho) and np.isfinite(w), (kind, delta, s)
            tol = 4 * EPS * float(rho0) + (4 * EPS * d / 3 if kind == "tukey" else 0.0)
            assert abs(rho - float(rho0)) <= tol, (kind, delta, s, rho, rho0)
            assert abs(w - float(w0)) <= 2 * EPS * float(w0), (kind, delta, s, w, w0)
            assert 0.0 <= w <= 1.0 and 0.0 <= rho <= s * (1 + 4 * EPS)


def test_huber_at_zero_and_every_kind_at_the_branch_point():
    for delta in DELTAS:
        d = delta * delta
        assert graph_robust_rho_w("huber", delta, 0.0) == (0.0, 1.0)
        for kind in ROBUST:
            lo, at, hi = (graph_robust_rho_w(kind, delta, s) for s in (d * (1 - 2.0 ** -52), d, d * (1 + 2.0 ** -52)))
            # rho is continuous at s = d: one ulp of s moves it by w ulp-of-s at most (w <= 1) plus the rounding of each side
            for a, b in ((lo, at), (at, hi)):
                assert abs(a[0] - b[0]) <= 4 * EPS * d, (kind, delta, a, b)
                assert abs(a[1] - b[1]) <= 4 * EPS, (kind, delta, a, b)
    assert graph_robust_rho_w("tukey", 1.0, 1.0)[1] == 0.0 and graph_robust_rho_w("tukey", 1.0, 2.0) == (1.0 / 3.0, 0.0)


@pytest.mark.parametrize("kind", ROBUST)
def test_w_is_the_derivative_of_rho(kind):
    """A central difference of the restatement's rho in extended precision (numpy.longdouble, 64-bit mantissa on x86-64), step h = 1e-6 s, at
    seeded s at least 1 % away from the branch point s = d.  Truncation: h^2 rho''' / 6 <= 1e-12 relative for these kernels (every derivative
    of rho falls at least as fast as rho / s^k); rounding: 2^-64 rho / h = 5e-14 rho / s.  The bound is 1e-9 relative to w, plus 1e-12 absolute
    where Tukey's w nears 0."""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is not extended precision here: the difference quotient needs it"
    rng = np.random.default_rng(67)
    for delta in DELTAS:
        d = delta * delta
        for s in d * 10.0 ** rng.uniform(-3, 3, size=60):
            if abs(s - d) < 0.01 * d:
                continue
            h = np.longdouble(1e-6) * np.longdouble(s)
            hi, lo = rr.rho_w(rr.KINDS[kind], delta, np.longdouble(s) + h, np.longdouble)[0], rr.rho_w(rr.KINDS[kind], delta, np.longdouble(s) - h, np.longdouble)[0]
            slope = float((hi - lo) / (2 * h))
            w = graph_robust_rho_w(kind, delta, float(s))[1]
            assert abs(w - slope) <= 1e-9 * abs(slope) + 1e-12, (kind, delta, s, w, slope)


def test_refusals_of_the_bare_function():
    from simpleslam_amd import PcrError
    for bad in ((7, 1.0, 1.0), (-1, 1.0, 1.0), ("huber", 0.0, 1.0), ("tukey", -1.0, 1.0), ("huber", np.inf, 1.0), ("huber", np.nan, 1.0),
                ("huber", 1.0, -1.0), ("none", 0.0, np.nan)):
        with pytest.raises(PcrError):
            graph_robust_rho_w(*bad)
    assert graph_robust_rho_w("none", 0.0, 3.0) == (3.0, 1.0)
    with pytest.raises(ValueError, match="unknown robust kernel"):
        graph_robust_rho_w("cauchy", 1.0, 1.0)


@pytest.mark.parametrize("kind", ("none",) + ROBUST)
def test_host_graph_equals_the_restatement_on_ring12_false(kind):
    """chi2 at the relative agreement test_graph_host.py's test_host_linearize_equals_graph_ref asserts for chi2 (1e-12); s at the same, w at
    1e-12 relative to 1 (w is a smooth function of s with |dw/ds| s <= 1 away from nothing: an error of 1e-12 in s moves it by less)."""
    g = rs.ring12_false()
    g.kind, g.delta = rr.KINDS[kind], rs.DELTA
    pg = rs.to_library(g, GRAPH_HOST)
    r, jf, jt, chi2 = pg.linearize()
    r0, jf0, jt0, _ = g.linearize()
    chi20 = g.chi2()
    assert np.abs(r - r0).max() < 1e-12 and np.abs(jf - jf0).max() < 1e-10 and np.abs(jt - jt0).max() < 1e-10      # unweighted, every factor
    assert abs(chi2 - chi20) <= 1e-12 * chi20, (chi2, chi20)
    s, w, marked, on = pg.betweenWeights()
    s0, w0 = g.between_weights()
    assert np.abs(s - s0).max() <= 1e-12 * s0.max() and np.abs(w - w0).max() <= 1e-12
    assert list(marked) == g.robust and on.all()
    if kind != "none":
        assert w[12] < 0.02 and w[:11].min() == 1.0       # the false loop at the start; odometry is never weighted
    # the false loop switched off: it leaves chi2 and stays in r, J and the readings
    pg.setBetweenEnabled(12, 1, False)
    g.enabled[12] = False
    r2, jf2, jt2, chi2_off = pg.linearize()
    assert np.array_equal(r2, r) and np.array_equal(jf2, jf) and np.array_equal(jt2, jt)
    assert abs(chi2_off - g.chi2()) <= 1e-12 * g.chi2() and chi2_off < chi2
    s2, w2, _, on2 = pg.betweenWeights()
    assert np.array_equal(s2, s) and np.array_equal(w2, w) and list(on2) == g.enabled


@pytest.fixture(scope="module")
def optima():
    """the restatement's optimum of ring12 (plain least squares) and of ring12_false under every kind, run until chi2 stalls"""
    base = rs.ring12()
    base.optimize(rel_tol=0.0, abs_tol=0.0)
    out = {"ring12": base}
    for name, kind in rr.KINDS.items():
        g = rs.ring12_false()
        g.kind, g.delta = kind, rs.DELTA
        g.optimize(rel_tol=0.0, abs_tol=0.0)
        out[name] = g
    return out


def test_the_scenes_separate_robust_from_plain(optima):
    """In the restatement alone, DELTA = 0.1, from the odometry chain.  Distance of pose 9 from its ring12 optimum, and the weights of the true
    loop (11 -> 0) and of the false loop (3 -> 9, off by 2 m and 40 degrees) at the optimum:
        none            8.540e-01 m   w 1       1
        huber           5.809e-02 m   w 1       1.538e-02
        geman_mcclure   1.436e-05 m   w 0.9856  4.568e-08
        tukey           1.440e-05 m   w 0.9855  0
    Plain least squares bends the ring by 85 cm; Huber, which never lets go, by a fifteenth of that; the two that redescend by 14 micrometres."""
    ref9 = optima["ring12"].poses[9]
    dist = {k: gr.pose_diff(optima[k].poses[9], ref9)[0] for k in rr.KINDS}
    print({k: f"{v:.3e}" for k, v in dist.items()})
    for kind in ROBUST:
        assert dist["none"] >= 10 * dist[kind], (kind, dist)
        s, w = optima[kind].between_weights()
        print(kind, f"w true {w[11]:.4f} false {w[12]:.3e}")
        if kind != "huber":
            assert w[12] < w[11], (kind, w[11], w[12])
    assert dist["none"] > 0.5 and dist["tukey"] < 1e-4 and dist["geman_mcclure"] < 1e-4
