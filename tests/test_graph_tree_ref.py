"""graph_tree_ref, the numpy restatement the tree preconditioner is held to, checked on its own: its block factorisation and sweeps solve
M z = r on every scene, M is what it claims to be, and the preconditioned conjugate gradient needs the iterations the issue's table records.

Backward error |Mz - r|_inf / (|M|_inf |z|_inf + |r|_inf) <= 1e-12, the bound of pcr_graph_apply's test: the backward error of a block
Cholesky does not grow with the conditioning (the forward error would).  Measured with this file over the eleven scenes and lambda in
{0, 1e-5, 10}: at most 4.2e-17, so the bound stands as stated."""
import numpy as np
import pytest

import graph_tree_ref as tr
import graph_tree_scenes as ts

LAMBDAS = (0.0, 1e-5, 10.0)
BOUND = 1e-12


@pytest.mark.parametrize("name", ts.NAMES)
def test_the_sweeps_solve_m(name):
    g = ts.scenes()[name]
    fr = tr.graph_forest(g)
    rng = np.random.default_rng(len(g.poses))
    r = rng.normal(size=6 * len(g.poses))
    for lam in LAMBDAS:
        M = tr.dense_m(g, lam, tr.TREE, fr)
        fac = tr.TreeFactor(g, lam, fr)
        assert fac.ok
        z = fac.solve(r)
        err = tr.backward_error(M, z, r)
        print(f"restated sweeps {name} lambda={lam}: backward error {err:.3e}")
        assert err <= BOUND, (name, lam, err)


@pytest.mark.parametrize("name", ["square-3", "star", "tree200", "two-components"])
def test_m_is_h_without_the_loops(name):
    """H + lam I - M is exactly the sum of the non-forest between factors: symmetric, positive semidefinite, of rank <= 6 per loop."""
    g = ts.scenes()[name]
    fr = tr.graph_forest(g)
    H, _, _ = g.normal_equations()
    E = H - tr.dense_m(g, 0.0, tr.TREE, fr)
    assert np.abs(E - E.T).max() <= 1e-9 * np.abs(H).max()
    w = np.linalg.eigvalsh((E + E.T) / 2)
    assert w.min() >= -1e-9 * np.abs(H).max()
    assert (w > 1e-9 * np.abs(H).max()).sum() <= 6 * fr["n_other"]
    touched = set()
    for e, (i, j, _, _) in enumerate(g.betweens):
        if not fr["in_tree"][e]:
            touched |= {i, j}
    for p in range(len(g.poses)):
        if p not in touched:
            assert not E[6 * p:6 * p + 6].any()


def test_the_forest_of_a_graph_without_loops_makes_pcg_one_step():
    g = ts.scenes()["n2"]
    it, capped = tr.first_solve_iterations(g, tr.TREE)
    assert (it, capped) == (1, False)


def test_iteration_counts_of_the_issues_table():
    """chain_graph(300): 11 iterations with the tree against 1 799 with the diagonal blocks at lambda 1e-5 (x0 = 0, |res| / |g| <= 1e-10)."""
    g = ts.scenes()["chain300"]
    tree, capped = tr.first_solve_iterations(g, tr.TREE)
    assert not capped and tree <= 13, tree
    jac, capped = tr.first_solve_iterations(g, tr.BLOCK_JACOBI)
    print(f"chain300 first solve: tree {tree}, block-Jacobi {jac}")
    assert not capped and jac > 16 * tree
