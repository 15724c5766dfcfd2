"""graph_ref, the numpy restatement of the pose graph, checked against itself: analytic Jacobians against central
differences, Exp / Log round trips, and a two-pose graph that must land on its measurement."""
import numpy as np
import pytest

import graph_ref as gr
import graph_scenes as gs

H = 1e-6


def _numeric(f, n_out=6):
    J = np.zeros((n_out, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = H
        J[:, k] = (f(d) - f(-d)) / (2 * H)
    return J


def _case(angle, seed):
    rng = np.random.default_rng(seed)
    Xi = gr.random_pose(rng, rng.uniform(0.2, 2.5), 50.0)
    Z = gr.random_pose(rng, rng.uniform(0.2, 2.5), 50.0)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    E = gr.exp(np.concatenate([axis * angle, rng.uniform(-50, 50, size=3)]))
    return Xi, Xi @ Z @ E, Z


@pytest.mark.parametrize("angle", gs.ANGLES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_between_jacobians_equal_central_differences(angle, seed):
    Xi, Xj, Z = _case(angle, seed)
    r, Ji, Jj = gr.between_jacobians(Xi, Xj, Z)
    assert abs(np.linalg.norm(r[:3]) - angle) < 1e-9
    Ni = _numeric(lambda d: gr.between_residual(Xi @ gr.exp(d), Xj, Z))
    Nj = _numeric(lambda d: gr.between_residual(Xi, Xj @ gr.exp(d), Z))
    for J, N in ((Ji, Ni), (Jj, Nj)):
        assert np.abs(J - N).max() <= 1e-6 * np.abs(J).max(), (angle, np.abs(J - N).max(), np.abs(J).max())


@pytest.mark.parametrize("angle", gs.ANGLES)
def test_prior_jacobian_equals_central_differences(angle):
    Xi, Xj, Z = _case(angle, 7)
    P = Xi @ Z
    r, J = gr.prior_jacobian(Xj, P)
    N = _numeric(lambda d: gr.prior_residual(Xj @ gr.exp(d), P))
    assert np.abs(J - N).max() <= 1e-6 * np.abs(J).max()


@pytest.mark.parametrize("angle", gs.ANGLES + (0.06, 3.1))
def test_exp_log_round_trip(angle):
    rng = np.random.default_rng(3)
    for _ in range(5):
        X = gr.random_pose(rng, angle, 50.0)
        assert np.abs(gr.exp(gr.log(X)) - X).max() < 1e-11 * 50
        xi = gr.log(X)
        assert abs(np.linalg.norm(xi[:3]) - angle) < 1e-9
        assert np.abs(gr.log(gr.exp(xi)) - xi).max() < 1e-10 * 50


def test_jr_inv_is_the_inverse_of_the_series_jacobian():
    """Jr = sum (-1)^n ad^n / (n + 1)!, summed until it stalls, times the closed-form inverse = I"""
    rng = np.random.default_rng(4)
    for angle in (1e-5, 0.3, 1.0, 2.5):
        xi = np.concatenate([rng.normal(size=3), rng.uniform(-5, 5, size=3)])
        xi[:3] *= angle / np.linalg.norm(xi[:3])
        a, term, Jr = gr.ad(xi), np.eye(6), np.eye(6)
        for n in range(1, 60):
            term = term @ (-a) / (n + 1)
            Jr = Jr + term
        assert np.abs(Jr @ gr.jr_inv(xi) - np.eye(6)).max() < 1e-10


def test_two_pose_graph_lands_on_its_measurement():
    rng = np.random.default_rng(9)
    X0 = gr.random_pose(rng, 0.7, 10.0)
    Z = gr.random_pose(rng, 0.4, 3.0)
    g = gr.Graph()
    g.poses = [X0 @ gr.exp(rng.normal(size=6) * 0.05), X0 @ Z @ gr.exp(rng.normal(size=6) * 0.05)]
    g.priors.append((0, X0, gr.NOISE["prior"]))
    g.betweens.append((0, 1, Z, gr.NOISE["odom"]))
    out = g.optimize(rel_tol=0.0, abs_tol=0.0)
    assert out["chi2_final"] < 1e-20
    assert np.abs(g.poses[0] - X0).max() < 1e-10
    assert np.abs(g.poses[1] - X0 @ Z).max() < 1e-10


def test_default_tolerances_report_convergence():
    name, g = gs.optimise_scenes()[0]
    out = g.optimize()
    assert out["converged"] and out["chi2_final"] < out["chi2_initial"]
