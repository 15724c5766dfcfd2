"""The small shapes at which the tree preconditioner can go wrong, as graph_ref.Graph objects: name -> graph, built once (scenes())."""
import functools

import numpy as np

import graph_ref as gr
import graph_scenes as gs


def _noisy(rng, T, trans, rot):
    return T @ gr.exp(np.concatenate([rng.normal(size=3) * rot, rng.normal(size=3) * trans]))


def build(truth, edges, priors, seed, trans=0.03, rot=np.deg2rad(2.0), meas=0.01):
    """truth: poses by id; edges: [(from, to, noise name)] in the order they are added; priors: ids.  Measurements carry a centimetre of noise,
    the estimates start a few centimetres and degrees off (the poses that hold a prior start on it), as graph_scenes.loop_graph does it."""
    rng = np.random.default_rng(seed)
    g = gr.Graph()
    g.poses = [T.copy() if k in priors else _noisy(rng, T, trans, rot) for k, T in enumerate(truth)]
    for k in priors:
        g.priors.append((k, truth[k].copy(), gr.NOISE["prior"]))
    for a, b, noise in edges:
        g.betweens.append((a, b, _noisy(rng, gr.inv(truth[a]) @ truth[b], meas, meas * 0.1), gr.NOISE[noise]))
    return g


def _walk(rng, n, parent_of):
    """truth poses: pose k = its parent's moved by a random step of up to 2 m and 0.2 rad"""
    truth = [np.eye(4)]
    for k in range(1, n):
        truth.append(truth[parent_of(k)] @ gr.random_pose(rng, rng.uniform(0.0, 0.2), 2.0))
    return truth


def single():
    return build([gr.random_pose(np.random.default_rng(1), 0.7, 5.0)], [], [0], 41)


def pair():
    rng = np.random.default_rng(2)
    return build(_walk(rng, 2, lambda k: k - 1), [(0, 1, "odom")], [0], 42)


def reversed_chain(n=40):
    """the path runs from id n - 1 down to id 0; every edge is added (i + 1 -> i), the prior holds id n - 1: every parent has a higher id than
    its child.  One loop from the far end back to the start."""
    rng = np.random.default_rng(3)
    along = _walk(rng, n, lambda k: k - 1)                 # along[s]: the s-th pose of the path
    truth = [along[n - 1 - k] for k in range(n)]           # id k sits at path step n - 1 - k
    edges = [(i + 1, i, "odom") for i in range(n - 2, -1, -1)] + [(0, n - 1, "loop")]
    return build(truth, edges, [n - 1], 43)


def star(leaves=64):
    """hub 0, `leaves` leaves, three leaf-to-leaf loops: depth 1, the leaves in round 0 and the hub in round 1"""
    rng = np.random.default_rng(4)
    truth = _walk(rng, leaves + 1, lambda k: 0)
    edges = [(0, k, "odom") for k in range(1, leaves + 1)] + [(3, 40, "loop"), (17, 5, "loop"), (64, 1, "loop")]
    return build(truth, edges, [0], 44)


def closest_keyframe_tree(n=200):
    """every pose tied to a random earlier one (Backend::addOdomFactor's mClosestKfIdx), four loops: one with from > to, one a duplicate of a
    tree edge (odometry noise and all)"""
    rng = np.random.default_rng(5)
    par = [0] + [int(rng.integers(0, k)) for k in range(1, n)]
    truth = _walk(rng, n, lambda k: par[k])
    edges = [(par[k], k, "odom") for k in range(1, n)]
    edges += [(12, 150, "loop"), (190, 30, "loop"), (par[77], 77, "odom"), (60, 199, "loop")]
    return build(truth, edges, [0], 45)


def two_components():
    """ids 0..9 and 10..24, a prior each; the second component's prior sits on id 17, not on its lowest id (10); one loop in each"""
    rng = np.random.default_rng(6)
    truth = _walk(rng, 25, lambda k: 0 if k == 10 else k - 1)
    edges = [(k - 1, k, "odom") for k in range(1, 10)] + [(k - 1, k, "odom") for k in range(11, 25)] + [(0, 9, "loop"), (24, 11, "loop")]
    return build(truth, edges, [0, 17], 46)


def inner_prior(n=30):
    """a chain with a second prior on an inner pose (priors touch diagonal blocks only, wherever they sit) and one loop"""
    rng = np.random.default_rng(7)
    truth = _walk(rng, n, lambda k: k - 1)
    edges = [(k - 1, k, "odom") for k in range(1, n)] + [(2, n - 1, "loop")]
    return build(truth, edges, [0, 19], 47)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> graph; built once and never modified (copy() before optimising)"""
    opt = dict(gs.optimise_scenes())
    return {
        "n1": single(),
        "n2": pair(),
        "square-3": opt["square-3"],
        "eight-3": opt["eight-3"],
        "chain300": gs.chain_graph(300),
        "reversed-chain": reversed_chain(),
        "star": star(),
        "tree200": closest_keyframe_tree(),
        "two-components": two_components(),
        "inner-prior": inner_prior(),
        "chain1025": gs.chain_graph(1025),
    }


NAMES = ("n1", "n2", "square-3", "eight-3", "chain300", "reversed-chain", "star", "tree200", "two-components", "inner-prior", "chain1025")
