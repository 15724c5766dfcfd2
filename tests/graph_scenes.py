"""Pose graphs the pcr_graph tests share: each builder returns a graph_ref.Graph; to_library() loads one into a simpleslam_amd.PoseGraph."""
import numpy as np

import graph_ref as gr

# rotation angle of the residual: the series at and near 0, 0.04 where only the library still takes its series (graph_ref's ends at 1e-3: the
# higher coefficients count there), the closed forms, near pi
ANGLES = (0.0, 1e-10, 1e-5, 0.04, 1.0, 3.0)


def full_info(rng):
    """a full symmetric positive definite information matrix"""
    a = rng.normal(size=(6, 6))
    return a @ a.T + 6 * np.eye(6)


def residual_graph(seed=11):
    """One prior and four between factors per angle of ANGLES, every residual with that rotation angle about a skew axis and a relative
    translation of up to 50 m, full information matrices."""
    rng = np.random.default_rng(seed)
    g = gr.Graph()
    for angle in ANGLES:
        for _ in range(4):
            Xi = gr.random_pose(rng, rng.uniform(0.2, 2.5), 50.0)
            Z = gr.random_pose(rng, rng.uniform(0.2, 2.5), 50.0)
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            E = gr.exp(np.concatenate([axis * angle, rng.uniform(-50, 50, size=3)]))
            i = len(g.poses)
            g.poses += [Xi, Xi @ Z @ E]
            g.betweens.append((i, i + 1, Z, full_info(rng)))
        P = gr.random_pose(rng, rng.uniform(0.2, 2.5), 50.0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        k = len(g.poses)
        g.poses.append(P @ gr.exp(np.concatenate([axis * angle, rng.uniform(-50, 50, size=3)])))
        g.priors.append((k, P, full_info(rng)))
    return g


def _perturb(rng, T, trans, rot):
    return T @ gr.exp(np.concatenate([rng.normal(size=3) * rot, rng.normal(size=3) * trans]))


def loop_graph(truth, loops, seed, trans=0.03, rot=np.deg2rad(2.0), meas_noise=0.01):
    """Odometry chain over `truth` with noisy measurements, `loops` = [(from, to)] loop edges, initial estimates perturbed by a few
    centimetres and degrees; the prior holds pose 0."""
    rng = np.random.default_rng(seed)
    g = gr.Graph()
    g.poses = [truth[0].copy()] + [_perturb(rng, T, trans, rot) for T in truth[1:]]
    g.priors.append((0, truth[0].copy(), gr.NOISE["prior"]))
    for i in range(len(truth) - 1):
        Z = _perturb(rng, gr.inv(truth[i]) @ truth[i + 1], meas_noise, meas_noise * 0.1)
        g.betweens.append((i, i + 1, Z, gr.NOISE["odom"]))
    for a, b in loops:
        Z = _perturb(rng, gr.inv(truth[a]) @ truth[b], meas_noise, meas_noise * 0.1)
        g.betweens.append((a, b, Z, gr.NOISE["loop"]))
    return g


def _planar(x, y, yaw, z=0.0):
    T = gr.exp(np.array([0.0, 0.0, yaw, 0.0, 0.0, 0.0]))
    T[:3, 3] = (x, y, z)
    return T


def square_truth():
    """8 poses around a 10 m square, heading along the path"""
    pts = [(0, 0), (5, 0), (10, 0), (10, 5), (10, 10), (5, 10), (0, 10), (0, 5)]
    out = []
    for k, (x, y) in enumerate(pts):
        nx, ny = pts[(k + 1) % 8]
        out.append(_planar(x, y, np.arctan2(ny - y, nx - x), 0.1 * k))
    return out


def eight_truth(n=65):
    """n poses along a figure of eight (a lemniscate 40 m across), heading along the path, with a gentle climb"""
    out = []
    for k in range(n):
        s = 2 * np.pi * k / (n - 1)
        x, y = 20 * np.sin(s), 10 * np.sin(2 * s)
        dx, dy = 20 * np.cos(s), 20 * np.cos(2 * s)
        out.append(_planar(x, y, np.arctan2(dy, dx), 0.05 * k))
    return out


def optimise_scenes():
    """(name, graph): the square with one and three loop edges, the figure of eight with one and three"""
    sq, e8 = square_truth(), eight_truth()
    return [
        ("square-1", loop_graph(sq, [(0, 7)], 21)),
        ("square-3", loop_graph(sq, [(0, 7), (1, 6), (0, 5)], 22)),
        ("eight-1", loop_graph(e8, [(0, 64)], 23)),
        ("eight-3", loop_graph(e8, [(0, 64), (0, 32), (32, 64)], 24)),
    ]


def product_graph(n, seed=5):
    """n poses for the product test: a chain, a hub (pose 0) with up to 40 loop edges, a duplicate edge, a pose that is only ever a "to" end
    (the last one), a prior on pose 0 and one on the middle pose; full information matrices, estimates off their measurements."""
    rng = np.random.default_rng(seed + n)
    g = gr.Graph()
    g.poses = [gr.random_pose(rng, rng.uniform(0.1, 2.0), 20.0) for _ in range(n)]
    g.priors.append((0, gr.random_pose(rng, 0.5, 20.0), full_info(rng)))
    if n > 2:
        g.priors.append((n // 2, g.poses[n // 2] @ gr.exp(rng.normal(size=6) * 0.1), full_info(rng)))

    def edge(i, j):
        Z = gr.inv(g.poses[i]) @ g.poses[j] @ gr.exp(rng.normal(size=6) * 0.2)
        g.betweens.append((i, j, Z, full_info(rng)))

    for i in range(n - 1):
        edge(i, i + 1)
    if n > 2:
        targets = rng.choice(np.arange(2, n), size=min(40, n - 2), replace=False)
        for t in targets:
            edge(0, int(t))
        edge(0, int(targets[0]))          # the duplicate
        edge(1, n - 1)                    # the last pose is never a "from" end
        g.betweens.append(g.betweens[1])  # a duplicate of a chain edge, measurement and all
    return g


def chain_graph(n=300, seed=31):
    """a chain of n poses along a gentle arc with one loop edge 0 -> n - 1"""
    truth = [_planar(2.0 * k * np.cos(0.002 * k), 2.0 * k * np.sin(0.002 * k), 0.004 * k) for k in range(n)]
    return loop_graph(truth, [(0, n - 1)], seed)


def to_library(g, device):
    """a simpleslam_amd.PoseGraph holding graph_ref.Graph g"""
    from simpleslam_amd.pcr import PoseGraph
    pg = PoseGraph(device=device)
    if g.poses:
        pg.addPoses(np.stack(g.poses))
    for k, P, Om in g.priors:
        pg.addPrior(P, k, Om)
    for i, j, Z, Om in g.betweens:
        pg.addBetween(i, j, Z, Om)
    return pg
