"""graph_fixed_ref, the numpy restatement of fixed poses, held to its own definition on the scenes of graph_fixed_scenes: at
its optimum the gradient over the free poses vanishes to rounding, fixed poses are untouched, and with nothing fixed it is graph_ref."""
import numpy as np
import pytest

import graph_fixed_ref as fr
import graph_fixed_scenes as fs
import graph_ref as gr
import graph_robust_ref as rr
import graph_robust_scenes as rs
import graph_scenes as gs

STALL = dict(rel_tol=0.0, abs_tol=0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def optima():
    """name -> (scene, optimised copy, result), computed once"""
    out = {}
    for name in fs.NAMES:
        g = fs.scenes()[name]
        ref = g.copy()
        out[name] = (g, ref, ref.optimize(**STALL))
    return out


@pytest.mark.parametrize("name", fs.NAMES)
def test_the_gradient_over_the_free_poses_vanishes_at_the_optimum(name, optima):
    g, ref, res = optima[name]
    H, grad, chi2, free = ref.reduced_equations()
    H0, grad0, chi20, _ = g.reduced_equations()
    # rounding: the gradient is a sum of J^T Omega r whose terms are each computed to an eps of their size; against the start's gradient it
    # has fallen by more than nine orders
    scale = np.abs(grad0).max()
    print(f"{name}: |g_free| {np.abs(grad).max():.3e} from {scale:.3e}; chi2 {chi20:.6g} -> {chi2:.6g}; {res}")
    assert np.abs(grad).max() <= 1e-9 * scale
    assert res["accepted"] > 0 and res["chi2_final"] < res["chi2_initial"] and abs(res["chi2_final"] - chi2) <= 1e-12 * max(chi2, 1.0)
    assert free.size == 6 * (len(g.poses) - len(g.fixed))
    # ... and it is a minimum of the reduced problem: H_ff is positive definite there
    assert np.linalg.eigvalsh(H).min() > 0
    # the full gradient is NOT zero on the fixed rows (they are constraints, not optima), or the scene would test nothing.  chain6 is the
    # exception by construction: without a prior the cost does not change when every pose moves together, so holding ONE pose only picks
    # the gauge and the full gradient vanishes with the reduced one
    full = ref.normal_equations()[1]
    fixed_rows = np.setdiff1d(np.arange(full.size), free)
    if name == "chain6":
        assert np.abs(full[fixed_rows]).max() <= 1e-9 * scale
    else:
        assert np.abs(full[fixed_rows]).max() > 1e3 * np.abs(grad).max()


@pytest.mark.parametrize("name", fs.NAMES)
def test_fixed_poses_are_untouched(name, optima):
    g, ref, _ = optima[name]
    moved = 0
    for p in range(len(g.poses)):
        if p in g.fixed:
            assert np.array_equal(_bits(g.poses[p]), _bits(ref.poses[p])), p
        else:
            moved += not np.array_equal(g.poses[p], ref.poses[p])
    assert moved == len(g.poses) - len(g.fixed)


@pytest.mark.parametrize("scene", ["square-3", "eight-1"])
def test_nothing_fixed_is_graph_ref_exactly(scene):
    g = dict(gs.optimise_scenes())[scene]
    a, b = g.copy(), fr.FixedGraph.of(g)
    ra, rb = a.optimize(**STALL), b.optimize(**STALL)
    assert ra == rb
    assert np.array_equal(_bits(np.stack(a.poses)), _bits(np.stack(b.poses)))


def test_nothing_fixed_is_the_robust_restatement_exactly():
    g = rs.ring12_false()
    g.kind, g.delta = rr.HUBER, rs.DELTA
    a, b = g.copy(), fr.FixedGraph.of(g)
    ra, rb = a.optimize(), b.optimize()
    assert ra == rb and np.array_equal(_bits(np.stack(a.poses)), _bits(np.stack(b.poses)))


def test_every_pose_fixed_returns_at_once():
    g = fr.FixedGraph.of(fs.scenes()["chain12"], range(12))
    before = [p.copy() for p in g.poses]
    res = g.optimize()
    assert res["iterations"] == 0 and res["converged"] and res["chi2_final"] == res["chi2_initial"] == g.normal_equations()[2] > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, g.poses))


def test_a_factor_between_two_fixed_poses_counts_in_chi2():
    g = fs.scenes()["chain12"]
    between_fixed = [e for e, (i, j, _, _) in enumerate(g.betweens) if i in g.fixed and j in g.fixed]
    assert len(between_fixed) == 3                          # 4-5, 5-6, 6-7
    without = g.copy()
    for e in between_fixed:
        without.enabled[e] = False
    assert g.chi2() > without.chi2() > 0
    # a constant term: the two problems have the same reduced equations, hence the same optimum
    Ha, ga, _, _ = g.reduced_equations()
    Hb, gb, _, _ = without.reduced_equations()
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb)


def test_the_scenes_are_the_shapes_they_claim():
    s = fs.scenes()
    assert not s["chain6"].priors and s["chain6"].fixed == {0} and len(s["chain6"].poses) == 6 and s["chain6"].betweens[-1][:2] == (5, 0)
    assert s["chain12"].fixed == {4, 5, 6, 7} and [k for k, _, _ in s["chain12"].priors] == [0]
    e8 = s["eight41"]
    crossing = [(i, j) for i, j, _, _ in e8.betweens[40:] if (i in e8.fixed) != (j in e8.fixed)]
    assert len(e8.poses) == 41 and len(e8.fixed) == 20 and len(e8.betweens) == 43 and len(crossing) == 2
    g70 = s["g70"]
    assert len(g70.poses) == 70 and {63, 64, 69} <= g70.fixed and len(g70.priors) + len(g70.betweens) > 256
    r = fs.ring12_false_into_fixed()
    assert r.betweens[12][:2] == rs.FALSE_LOOP and rs.FALSE_LOOP[1] in r.fixed and r.robust[12]
