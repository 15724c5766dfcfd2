"""pcr_graph's robust kernels on the GPU: every instantiation of the linearise kernel against a host graph bit for bit, the
solve's product against the restatement's weighted H, the optimiser against the restatement's dense Levenberg-Marquardt under both
preconditioners, the way from the verdict to the switch, and that marks change no bit under the defaults."""
import numpy as np
import pytest

import graph_ref as gr
import graph_robust_ref as rr
import graph_robust_scenes as rs
from simpleslam_amd.pcr import GRAPH_HOST

pytestmark = pytest.mark.gpu

KINDS = ("none", "huber", "geman_mcclure", "tukey")

# Optimum agreement on ring12_false, device against the restatement's dense LM from the same start, both under the default tolerances:
#   1. the restatement against itself at lambda_init 1e-5 and 1e-3: 6.291e-07 m, 3.581e-08 rad (the largest over the four kinds; under "none")
#   2. what test_graph_gpu.py allows the plain optimiser against graph_ref: 2.2e-09 m, 1.2e-10 rad
#   3. ten times the larger of the two: the two solvers stop on different steps of a flat basin
SPREAD_T, SPREAD_R = 6.291e-07, 3.581e-08
PLAIN_T, PLAIN_R = 2.2e-09, 1.2e-10
BOUND_T, BOUND_R = 10 * max(SPREAD_T, PLAIN_T), 10 * max(SPREAD_R, PLAIN_R)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(dev, host, what):
    for name, a, b in zip(("r", "J_from", "J_to"), dev.linearize()[:3], host.linearize()[:3]):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, np.abs(a - b).max())
    cd, ch = dev.linearize()[3], host.linearize()[3]
    assert np.float64(cd).view(np.uint64) == np.float64(ch).view(np.uint64), (what, cd, ch)
    wd, wh = dev.betweenWeights(), host.betweenWeights()
    for name, a, b in zip(("s", "w"), wd[:2], wh[:2]):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, a, b)
    assert np.array_equal(wd[2], wh[2]) and np.array_equal(wd[3], wh[3])
    return cd, wd


def _worst(A, B):
    d = [gr.pose_diff(a, b) for a, b in zip(A, B)]
    return max(x[0] for x in d), max(x[1] for x in d)


@pytest.fixture(scope="module")
def references():
    """the restatement's dense LM under the default tolerances: ring12 under plain least squares, ring12_false under every kind"""
    base = rs.ring12()
    base.optimize()
    out = {"ring12": base.poses}
    for kind in KINDS:
        g = rs.ring12_false()
        g.kind, g.delta = rr.KINDS[kind], rs.DELTA
        g.optimize()
        out[kind] = g.poses
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_factors", rs.FOLD_SIZES)
def test_linearize_equals_the_host_on_the_fold_edges(kind, n_factors):
    g = rs.fold_graph(n_factors)
    g.kind, g.delta = rr.KINDS[kind], rs.FOLD_DELTA
    g.enabled[n_factors // 2] = False                     # a disabled factor in the middle
    dev, host = rs.to_library(g, 0), rs.to_library(g, GRAPH_HOST)
    assert dev.size()[1] + dev.size()[2] == n_factors
    chi2, (s, w, marked, on) = _same_bits(dev, host, (kind, n_factors))
    assert abs(chi2 - g.chi2()) <= 1e-12 * chi2
    assert (w[~marked] == 1.0).all()
    wm = w[marked]                                        # both sides of delta^2 occur among the marked factors
    if kind == "huber":
        assert (wm == 1.0).any() and (wm < 1.0).any()
    if kind == "tukey":
        assert (wm == 0.0).any() and ((wm > 0.0) & (wm < 1.0)).any()
    if kind == "geman_mcclure":
        assert (wm < 1.0).all() and (wm > 0.0).all()
    assert not on[n_factors // 2] and on.sum() == len(on) - 1


@pytest.mark.parametrize("kind", KINDS)
def test_linearize_equals_the_host_on_the_small_graphs(kind):
    k = rr.KINDS[kind]
    for name, g in (("ring12_false", rs.ring12_false()), ("prior alone", rs.prior_alone()), ("two poses", rs.two_poses()),
                    ("zero residual", rs.two_poses(exact=True))):
        g.kind, g.delta = k, rs.DELTA
        dev, host = rs.to_library(g, 0), rs.to_library(g, GRAPH_HOST)
        chi2, (s, w, marked, on) = _same_bits(dev, host, (kind, name))
        if name == "zero residual":
            assert s[0] == 0.0 and w[0] == 1.0, (kind, s, w)          # Huber at s = 0: no division
        if name == "ring12_false":
            dev.setBetweenEnabled(12, 1, False)
            host.setBetweenEnabled(12, 1, False)
            off, _ = _same_bits(dev, host, (kind, name, "off"))
            assert off < chi2


@pytest.mark.parametrize("kind", KINDS)
def test_apply_equals_the_weighted_dense_product(kind):
    """at the agreement test_graph_gpu.py's test_apply_equals_the_dense_product asserts for the plain product: 1e-12 relative to the largest entry"""
    g = rs.ring12_false()
    g.kind, g.delta = rr.KINDS[kind], rs.DELTA
    g.enabled[4] = False
    g.add_between(2, 7, gr.inv(g.poses[2]) @ g.poses[7], gr.NOISE["loop"])      # a second link across, so that the graph stays one component
    pg = rs.to_library(g, 0)
    H, _, _ = g.normal_equations()
    x = np.random.default_rng(71).normal(size=6 * len(g.poses))
    for lam in (0.0, 1e-5, 10.0):
        y = pg.apply(lam, x)
        want = H @ x + lam * x
        err = np.abs(y - want).max() / np.abs(want).max()
        print(f"apply {kind} lambda={lam}: relative error {err:.3e}")
        assert err <= 1e-12, (kind, lam, err)


@pytest.mark.parametrize("precond", ("block_jacobi", "tree"))
@pytest.mark.parametrize("kind", KINDS)
def test_optimize_reaches_the_restatements_optimum(kind, precond, references):
    g = rs.ring12_false()
    g.kind, g.delta = rr.KINDS[kind], rs.DELTA
    pg = rs.to_library(g, 0)
    out = pg.optimize(pcg_preconditioner=precond)
    dt, dr = _worst(pg.poses(), references[kind])
    s, w, _, _ = pg.betweenWeights()
    print(f"optimize {kind} {precond}: |dt| {dt:.3e} m |dR| {dr:.3e} rad; w true {w[11]:.4f} false {w[12]:.3e}; {out}")
    assert dt <= BOUND_T and dr <= BOUND_R, (kind, precond, dt, dr)
    assert out.pcg_capped == 0 and out.converged
    assert out.accepted > 0 and out.chi2_final < out.chi2_initial
    if kind in ("geman_mcclure", "tukey"):
        assert w[12] < 1e-6 < w[11]


def test_from_the_verdict_to_the_switch(references):
    g = rs.ring12_false()
    pg = rs.to_library(g, 0)
    first = pg.optimize()
    assert first.converged
    bent = gr.pose_diff(pg.poses()[9], references["ring12"][9])[0]
    assert bent > 0.5                                     # plain least squares believed the false loop
    again = pg.optimize()
    assert again.iterations == 0                          # nothing new ...
    s, w, marked, on = pg.betweenWeights()
    worst = int(np.argmax(s))
    assert worst == 12 and marked[worst]
    pg.setBetweenEnabled(worst, 1, False)
    second = pg.optimize()                                # ... until the switch: real work
    assert second.iterations > 0 and second.accepted > 0 and second.converged and second.pcg_capped == 0
    dt, dr = _worst(pg.poses(), references["ring12"])
    print(f"after the switch: |dt| {dt:.3e} m |dR| {dr:.3e} rad; {second}")
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)


def test_marks_change_no_bit_under_the_defaults():
    g = rs.ring12_false()
    a, b = rs.to_library(g, 0), rs.to_library(g, 0, marks=False)
    assert a.betweenWeights()[2].sum() == 2 and not b.betweenWeights()[2].any()
    ra, rb = a.optimize(), b.optimize()
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    assert (ra.iterations, ra.accepted, ra.pcg_iterations, ra.chi2_final) == (rb.iterations, rb.accepted, rb.pcg_iterations, rb.chi2_final)
    a.setRobustKernel("tukey", rs.DELTA)                  # the kernel is something new: the early return does not fire
    assert a.optimize().iterations > 0
