"""Scenes of the robust-kernel tests: each builder returns a graph_robust_ref.RobustGraph; to_library() loads one into a PoseGraph."""
import numpy as np

import graph_ref as gr
import graph_robust_ref as rr
import graph_scenes as gs

# The kernel width the ring scenes are optimised under, in units of a residual's Mahalanobis length (d = DELTA^2 = 0.01).  At the start, the
# odometry chain, the true loop's s is 4.6e-3 (inside d: Tukey keeps it) and the false loop's 47 (4.7e3 d); at the robust optima the true
# loop's falls to 7e-5 and the false loop's stays at 42 to 47.  The odometry noise is what sets the first figure: with a centimetre per edge
# the chain drifts until the true loop starts beyond d, and Tukey gives it no weight from the first step on.
DELTA = 0.1
ODOM_NOISE_M, ODOM_NOISE_RAD = 0.002, 0.0002
FALSE_LOOP = (3, 9)                  # its index among the between factors is 12: eleven odometry edges, then the true loop
FALSE_OFFSET_M, FALSE_OFFSET_DEG = 2.0, 40.0


def _ring_truth(n=12, radius=10.0):
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        out.append(gs._planar(radius * np.cos(a), radius * np.sin(a), a + np.pi / 2, 0.02 * k))
    return out


def ring12(false_loop=False, seed=41):
    """Twelve poses on a circle of 10 m radius: odometry edges with 2 mm and 0.2 mrad of seeded noise, the true loop 11 -> 0 and,
    with false_loop, a loop 3 -> 9 whose measurement is wrong by 2 m and 40 degrees.  Both loops are marked.  The start is the odometry chain
    composed from pose 0 (the kernels that redescend end where the start sends them, so the start is part of the scene)."""
    rng = np.random.default_rng(seed)
    truth = _ring_truth()
    g = rr.RobustGraph()
    g.priors.append((0, truth[0].copy(), gr.NOISE["prior"]))
    g.poses = [truth[0].copy()]
    for i in range(11):
        Z = gs._perturb(rng, gr.inv(truth[i]) @ truth[i + 1], ODOM_NOISE_M, ODOM_NOISE_RAD)
        g.add_between(i, i + 1, Z, gr.NOISE["odom"])
        g.poses.append(g.poses[-1] @ Z)
    g.add_loop(11, 0, gs._perturb(rng, gr.inv(truth[11]) @ truth[0], 0.01, 0.001), gr.NOISE["loop"])
    if false_loop:
        a, b = FALSE_LOOP
        wrong = gr.exp(np.array([0.0, 0.0, np.deg2rad(FALSE_OFFSET_DEG), 0.0, 0.0, 0.0]))
        wrong[:3, 3] = (FALSE_OFFSET_M, 0.0, 0.0)
        g.add_loop(a, b, gr.inv(truth[a]) @ truth[b] @ wrong, gr.NOISE["loop"])
    return g


def ring12_false():
    return ring12(True)


FOLD_SIZES = (63, 64, 65, 256, 257)      # factors in total: the wave and block edges of the chi2 fold
FOLD_DELTA = 0.3                         # the marked factors' s runs from 0.1 to 4 times its square: both branches of every kernel are taken


def fold_graph(n_factors, seed=43):
    """A chain with n_factors factors in total (one prior, n_factors - 1 odometry edges), every fifth between factor marked, estimates a few
    centimetres and a fraction of a degree off their measurements, full information matrices."""
    rng = np.random.default_rng(seed + n_factors)
    n = n_factors
    truth = [gs._planar(2.0 * k * np.cos(0.01 * k), 2.0 * k * np.sin(0.01 * k), 0.02 * k) for k in range(n)]
    g = rr.RobustGraph()
    g.priors.append((0, truth[0].copy(), gr.NOISE["prior"]))
    g.poses = [truth[0].copy()] + [gs._perturb(rng, T, 0.03, np.deg2rad(0.3)) for T in truth[1:]]
    for i in range(n - 1):
        Z = gs._perturb(rng, gr.inv(truth[i]) @ truth[i + 1], 0.01, 0.001)
        g.add_between(i, i + 1, Z, gs.full_info(rng), robust=(i % 5 == 0))
    return g


def prior_alone():
    """one pose, one prior: a one-factor graph"""
    rng = np.random.default_rng(47)
    g = rr.RobustGraph()
    P = gr.random_pose(rng, 0.7, 5.0)
    g.poses = [P @ gr.exp(rng.normal(size=6) * 0.1)]
    g.priors.append((0, P, gs.full_info(rng)))
    return g


def two_poses(exact=False):
    """two poses, a prior and one marked between factor; exact: the measurement is X_0^-1 X_1 of poses for which the library's residual is
    zero to the last bit (identity rotations, translations that subtract exactly), the case where Huber takes s = 0"""
    rng = np.random.default_rng(53)
    g = rr.RobustGraph()
    if exact:
        A, B, Z = np.eye(4), np.eye(4), np.eye(4)
        A[:3, 3], B[:3, 3], Z[:3, 3] = (1.0, 2.0, -0.5), (3.5, 2.25, 4.0), (2.5, 0.25, 4.5)
    else:
        A = gr.random_pose(rng, 0.4, 5.0)
        Z = gr.random_pose(rng, 0.9, 3.0)
        B = A @ Z @ gr.exp(rng.normal(size=6) * 0.3)
    g.poses = [A, B]
    g.priors.append((0, A @ gr.exp(rng.normal(size=6) * 0.01), gs.full_info(rng)))
    g.add_loop(0, 1, Z, gs.full_info(rng))
    return g


def to_library(g, device, kind=None, delta=None, marks=True):
    """a PoseGraph holding RobustGraph g: marked factors through addLC, the rest through addBetween, then the switches and the kernel
    (kind / delta override the graph's own; marks=False loads every factor unmarked)"""
    from simpleslam_amd.pcr import PoseGraph
    pg = PoseGraph(device=device)
    if g.poses:
        pg.addPoses(np.stack(g.poses))
    for k, P, Om in g.priors:
        pg.addPrior(P, k, Om)
    for e, (i, j, Z, Om) in enumerate(g.betweens):
        (pg.addLC if (g.robust[e] and marks) else pg.addBetween)(i, j, Z, Om)
    for e, on in enumerate(g.enabled):
        if not on:
            pg.setBetweenEnabled(e, 1, False)
    kind = g.kind if kind is None else kind
    if kind != rr.NONE:
        pg.setRobustKernel(kind, g.delta if delta is None else delta)
    return pg
