"""The tree preconditioner on the GPU: pcr_graph_precondition against numpy's dense M for both kinds, the solve's iteration
counts against graph_tree_ref's conjugate gradient, the optimum against graph_ref's dense-solve Levenberg-Marquardt, run-to-run identity,
the forest of a graph that grows, and the default left as it was."""
import numpy as np
import pytest

import graph_ref as gr
import graph_scenes as gs
import graph_tree_ref as tr
import graph_tree_scenes as ts
from simpleslam_amd import PoseGraph
from simpleslam_amd.pcr import GRAPH_PRECOND_BLOCK_JACOBI, GRAPH_PRECOND_TREE

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 1e-5, 10.0)
BACKWARD = 1e-12           # |Mz - r|_inf / (|M|_inf |z|_inf + |r|_inf): the bound of pcr_graph_apply's test
# The device's PCG iterations of one solve against graph_tree_ref's (numpy sums in another order than block_sum): measured on an MI355X over
# the eleven scenes, the largest difference was MEASURED_IT_DIFF (profiles/graph_tree_notes.md); the test allows twice that, at least 2.
MEASURED_IT_DIFF = 1
IT_MARGIN = max(2, 2 * MEASURED_IT_DIFF)
# the bounds tests/test_graph_gpu.py holds block-Jacobi to: ten times the largest distance measured over its four scenes
BOUND_T, BOUND_R = 2.2e-9, 1.2e-10
STALL = dict(rel_tol=0.0, abs_tol=0.0, pcg_rel_tol=1e-14)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _worst(A, B):
    d = [gr.pose_diff(a, b) for a, b in zip(A, B)]
    return max(x[0] for x in d), max(x[1] for x in d)


@pytest.mark.parametrize("name", ts.NAMES)
def test_precondition_tree_solves_m(name):
    g = ts.scenes()[name]
    fr = tr.graph_forest(g)
    pg = gs.to_library(g, 0)
    r = np.random.default_rng(len(g.poses)).normal(size=6 * len(g.poses))
    for lam in LAMBDAS:          # lambda = 0 is legal: every component holds a prior
        M = tr.dense_m(g, lam, tr.TREE, fr)
        z = pg.precondition(lam, r, GRAPH_PRECOND_TREE)
        err = tr.backward_error(M, z, r)
        print(f"precondition tree {name} lambda={lam}: backward error {err:.3e}")
        assert np.isfinite(z).all() and err <= BACKWARD, (name, lam, err)
    assert np.array_equal(_bits(pg.precondition(10.0, r, "tree")), _bits(z))          # the same bits run to run


@pytest.mark.parametrize("name", ts.NAMES)
def test_precondition_block_jacobi_solves_the_block_diagonal(name):
    g = ts.scenes()[name]
    pg = gs.to_library(g, 0)
    r = np.random.default_rng(len(g.poses)).normal(size=6 * len(g.poses))
    for lam in LAMBDAS:
        M = tr.dense_m(g, lam, tr.BLOCK_JACOBI)
        z = pg.precondition(lam, r, GRAPH_PRECOND_BLOCK_JACOBI)
        err = tr.backward_error(M, z, r)
        print(f"precondition block-Jacobi {name} lambda={lam}: backward error {err:.3e}")
        assert np.isfinite(z).all() and err <= BACKWARD, (name, lam, err)


@pytest.mark.parametrize("name", ts.NAMES)
def test_one_solve_takes_the_restated_number_of_iterations(name):
    g = ts.scenes()[name]
    want, capped = tr.first_solve_iterations(g, tr.TREE, lam=1e-5, tol=1e-10)
    assert not capped
    out = gs.to_library(g, 0).optimize(max_iterations=1, pcg_rel_tol=1e-10, pcg_preconditioner="tree")
    print(f"one solve {name}: device {out.pcg_iterations} iterations, restated {want}, difference {out.pcg_iterations - want}")
    assert out.iterations == 1 and out.pcg_capped == 0
    assert abs(out.pcg_iterations - want) <= IT_MARGIN, (name, out.pcg_iterations, want)


def test_the_tree_needs_a_tenth_of_the_iterations_on_a_chain():
    """A condition, not a measurement: graph_tree_ref gives 11 against 1 799 on chain_graph(300), a factor 16 inside it."""
    g = ts.scenes()["chain300"]
    tree = gs.to_library(g, 0).optimize(max_iterations=1, pcg_rel_tol=1e-10, pcg_preconditioner=GRAPH_PRECOND_TREE)
    jac = gs.to_library(g, 0).optimize(max_iterations=1, pcg_rel_tol=1e-10, pcg_preconditioner=GRAPH_PRECOND_BLOCK_JACOBI)
    print(f"chain300 first solve: tree {tree.pcg_iterations}, block-Jacobi {jac.pcg_iterations}")
    assert tree.pcg_capped == 0 and jac.pcg_capped == 0
    assert 10 * tree.pcg_iterations < jac.pcg_iterations
    assert tree.chi2_final < tree.chi2_initial and abs(tree.chi2_final - jac.chi2_final) <= 1e-6 * jac.chi2_final


def _optimum_scenes():
    return list(gs.optimise_scenes()) + [("tree200", ts.scenes()["tree200"])]


@pytest.fixture(scope="module")
def references():
    """graph_ref's optimum of every scene (dense solves, run to a stall), computed once: name -> (graph before, optimised poses, result)"""
    out = {}
    for name, g in _optimum_scenes():
        ref = g.copy()
        res = ref.optimize(rel_tol=0.0, abs_tol=0.0)
        out[name] = (g, ref.poses, res)
    return out


@pytest.mark.parametrize("name", ["square-1", "square-3", "eight-1", "eight-3", "tree200"])
def test_optimize_with_the_tree_reaches_graph_refs_minimum(name, references):
    g, ref_poses, ref = references[name]
    pg = gs.to_library(g, 0)
    out = pg.optimize(pcg_preconditioner="tree", **STALL)
    dt, dr = _worst(pg.poses(), ref_poses)
    print(f"optimize tree {name}: |dt| {dt:.3e} m |dR| {dr:.3e} rad; chi2 {out.chi2_final:.12g} vs {ref['chi2_final']:.12g}; {out}")
    assert out.accepted > 0 and out.pcg_iterations > 0 and out.chi2_final < out.chi2_initial
    assert dt <= BOUND_T and dr <= BOUND_R, (name, dt, dr)


def test_run_to_run_is_bit_identical():
    g = ts.scenes()["tree200"]
    runs = []
    for _ in range(2):
        pg = gs.to_library(g, 0)
        out = pg.optimize(pcg_preconditioner="tree")
        runs.append((out.iterations, out.accepted, out.pcg_iterations, out.chi2_final, np.ascontiguousarray(pg.poses()).tobytes()))
    assert runs[0] == runs[1]
    assert runs[0][2] > 0


def test_a_graph_that_grows_ends_where_one_batch_ends(references):
    """optimHandler's pattern under the tree: every key frame arrives with its odometry factor and is optimised, then the loops.  The forest
    is planned anew whenever factors arrived; a stale one would leave new poses out of M."""
    g, ref_poses, _ = references["eight-3"]
    n = len(g.poses)
    chain, loops = g.betweens[:n - 1], g.betweens[n - 1:]
    batch = gs.to_library(g, 0)
    batch.optimize(pcg_preconditioner="tree", **STALL)
    inc = PoseGraph(device=0)
    inc.addPrior(g.priors[0][1], 0, g.priors[0][2])
    inc.addEstimate(0, g.poses[0])
    for k in range(1, n):
        inc.addEstimate(k, g.poses[k])
        inc.addBetween(k - 1, k, chain[k - 1][2], chain[k - 1][3])
        out = inc.optimize(pcg_preconditioner="tree")
        assert out.pcg_capped == 0
        parent, n_tree, n_other = inc.tree()
        assert (n_tree, n_other) == (k, 0) and parent[k] == k - 1
    for i, j, Z, Om in loops:
        inc.addLC(i, j, Z, Om)
    out = inc.optimize(pcg_preconditioner="tree", **STALL)
    assert inc.tree()[1:] == (n - 1, len(loops))
    dt, dr = _worst(inc.poses(), batch.poses())
    print(f"tree, incremental against batch: |dt| {dt:.3e} m |dR| {dr:.3e} rad; {out}")
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)
    dt, dr = _worst(inc.poses(), ref_poses)
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)


def test_the_default_is_the_block_diagonal_as_before():
    g = ts.scenes()["eight-3"]
    a, b = gs.to_library(g, 0), gs.to_library(g, 0)
    ra, rb = a.optimize(), b.optimize(pcg_preconditioner="block_jacobi")
    assert (ra.iterations, ra.accepted, ra.pcg_iterations, ra.pcg_capped) == (rb.iterations, rb.accepted, rb.pcg_iterations, rb.pcg_capped)
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    c = gs.to_library(g, 0)
    rc = c.optimize(pcg_preconditioner="tree")
    assert rc.pcg_iterations < ra.pcg_iterations          # another preconditioner did run
