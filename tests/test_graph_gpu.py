"""pcr_graph on the GPU: the linearisation against the host's bit for bit, the solve kernel's product against graph_ref's dense
H + lambda I, the optimiser against graph_ref's Levenberg-Marquardt with a dense solve, the cap, run-to-run identity, the way into the
key-frame store and optimHandler's incremental pattern."""
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_ref as gr
import graph_scenes as gs
from simpleslam_amd import PcrError, PoseGraph, SubMap
from simpleslam_amd.pcr import GRAPH_HOST

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Device against graph_ref after both ran until chi2 stalled (LM tolerances 0, pcg_rel_tol 1e-14), measured on an MI355X (m, rad):
#   square-1 5.5e-13 3.6e-14   square-3 5.1e-12 1.1e-12   eight-1 6.6e-11 3.2e-12   eight-3 2.2e-10 1.2e-11
#   (the incremental builds against one batch optimisation of eight-3: 5.2e-10 2.6e-11 with add_between, 4.5e-10 1.9e-11 with add_between_poses)
MEASURED_T, MEASURED_R = 2.2e-10, 1.2e-11      # the largest over the four scenes
# The bound is ten times that (the factor covers the other machines of the pool; a PCG stopped at a residual tolerance is not a dense
# solve, so no tighter figure can be derived) and may never exceed 1e-6 m / 1e-6 rad, a hundredth of the project's pose contract.
BOUND_T, BOUND_R = min(10 * MEASURED_T, 1e-6), min(10 * MEASURED_R, 1e-6)
STALL = dict(rel_tol=0.0, abs_tol=0.0, pcg_rel_tol=1e-14)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _worst(A, B):
    d = [gr.pose_diff(a, b) for a, b in zip(A, B)]
    return max(x[0] for x in d), max(x[1] for x in d)


@pytest.fixture(scope="module")
def references():
    """graph_ref's optimum of every scene, computed once: name -> (graph before, optimised poses, result dict)"""
    out = {}
    for name, g in gs.optimise_scenes():
        ref = g.copy()
        res = ref.optimize(rel_tol=0.0, abs_tol=0.0)
        out[name] = (g, ref.poses, res)
    return out


@pytest.mark.parametrize("scene", ["residual", "product65", "chain300"])
def test_linearize_equals_the_host_bit_for_bit(scene):
    g = {"residual": gs.residual_graph, "product65": lambda: gs.product_graph(65), "chain300": gs.chain_graph}[scene]()
    dev, host = gs.to_library(g, 0).linearize(), gs.to_library(g, GRAPH_HOST).linearize()
    for name, a, b in zip(("r", "J_from", "J_to"), dev, host):
        assert np.array_equal(_bits(a), _bits(b)), (name, np.abs(a - b).max())
    assert np.float64(dev[3]).view(np.uint64) == np.float64(host[3]).view(np.uint64), (dev[3], host[3])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025])
def test_apply_equals_the_dense_product(n):
    g = gs.product_graph(n)
    if n > 2:
        deg = np.bincount([i for i, j, _, _ in g.betweens] + [j for i, j, _, _ in g.betweens], minlength=n)
        assert deg[0] >= 40 and all(i != n - 1 for i, _, _, _ in g.betweens)          # the hub; a pose that is only ever a "to" end
        assert sum(1 for e in g.betweens if e[:2] == g.betweens[1][:2]) == 2           # the duplicate edge
    pg = gs.to_library(g, 0)
    H, _, _ = g.normal_equations()
    rng = np.random.default_rng(n)
    x = rng.normal(size=6 * n)
    for lam in (0.0, 1e-5, 10.0):
        y = pg.apply(lam, x)
        want = H @ x + lam * x
        err = np.abs(y - want).max() / np.abs(want).max()
        print(f"apply n={n} lambda={lam}: relative error {err:.3e}")
        assert err <= 1e-12, (n, lam, err)


@pytest.mark.parametrize("scene", ["square-1", "square-3", "eight-1", "eight-3"])
def test_optimize_reaches_graph_refs_minimum(scene, references):
    g, ref_poses, ref = references[scene]
    pg = gs.to_library(g, 0)
    out = pg.optimize(**STALL)
    dt, dr = _worst(pg.poses(), ref_poses)
    print(f"optimize {scene}: |dt| {dt:.3e} m |dR| {dr:.3e} rad; chi2 {out.chi2_final:.12g} vs {ref['chi2_final']:.12g}; {out}")
    assert dt <= BOUND_T and dr <= BOUND_R, (scene, dt, dr)
    assert abs(out.chi2_initial - ref["chi2_initial"]) <= 1e-11 * ref["chi2_initial"]
    # chi2 at a point within the bound of graph_ref's: first and second order terms of the difference, from graph_ref's own H and g there
    H, grad, _ = g.normal_equations(ref_poses)
    B = max(BOUND_T, BOUND_R)
    slack = 2 * np.abs(grad).sum() * B + np.linalg.norm(H, 2) * 6 * len(g.poses) * B * B + 1e-12 * ref["chi2_final"]
    assert out.chi2_final <= ref["chi2_final"] + slack, (out.chi2_final, ref["chi2_final"], slack)
    assert out.pcg_iterations > 0 and out.accepted > 0 and out.chi2_final < out.chi2_initial


@pytest.mark.parametrize("scene", ["square-1", "square-3", "eight-1", "eight-3"])
def test_default_parameters_converge(scene, references):
    g, ref_poses, ref = references[scene]
    pg = gs.to_library(g, 0)
    out = pg.optimize()
    assert out.converged and out.pcg_capped == 0 and out.chi2_final < out.chi2_initial
    dt, dr = _worst(pg.poses(), ref_poses)
    assert dt < 1e-3 and dr < 1e-3          # GTSAM's default tolerances stop early; the estimate is at the same minimum
    # delta = X_last after * X_last before^-1, re-orthonormalised
    d = pg.poses()[-1] @ gr.inv(g.poses[-1])
    assert np.abs(out.delta - d).max() < 1e-12 and np.abs(out.delta[:3, :3] @ out.delta[:3, :3].T - np.eye(3)).max() < 1e-15


def test_the_cap_is_reported():
    g = gs.chain_graph()
    pg = gs.to_library(g, 0)
    out = pg.optimize(pcg_max_iterations=20)
    assert out.pcg_capped > 0 and out.chi2_final <= out.chi2_initial
    assert out.pcg_iterations <= 20 * out.iterations
    pg = gs.to_library(g, 0)
    out = pg.optimize()
    assert out.converged and out.pcg_capped == 0 and out.chi2_final < out.chi2_initial


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graph_scenes as gs
name, g = gs.optimise_scenes()[3]
pg = gs.to_library(g, 0)
out = pg.optimize()
print(out.iterations, out.accepted, out.pcg_iterations, np.ascontiguousarray(pg.poses()).tobytes().hex())
'''


def test_run_to_run_is_bit_identical():
    name, g = gs.optimise_scenes()[3]
    runs = []
    for _ in range(2):
        pg = gs.to_library(g, 0)
        out = pg.optimize()
        runs.append((out.iterations, out.accepted, out.pcg_iterations, np.ascontiguousarray(pg.poses()).tobytes().hex()))
    assert runs[0] == runs[1]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    child = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=120, env=env)
    assert child.returncode == 0, child.stderr
    it, acc, pcg, hexed = child.stdout.split()
    assert (int(it), int(acc), int(pcg), hexed) == runs[0]


def test_into_the_key_frame_store():
    name, g = gs.optimise_scenes()[1]
    n = len(g.poses)
    rng = np.random.default_rng(1)
    a, b = SubMap(device=0), SubMap(device=0)
    for m in (a, b):
        for k in range(n):
            m.addKeyFrame(rng.normal(size=(16, 4)).astype(np.float32), g.poses[k])
    pg = gs.to_library(g, 0)
    pg.optimize()
    gen = a.generation()
    pg.applyTo(a)
    assert a.generation() == gen                         # as pcr_map_set_poses: no generation moves
    b.setPoses(0, pg.poses())
    for k in range(n):
        assert np.array_equal(_bits(a.keyFrame(k)[1]), _bits(b.keyFrame(k)[1])), k
    pg.applyTo(a, 2, 3)                                  # a range
    with pytest.raises(PcrError, match="different devices"):
        gs.to_library(g, GRAPH_HOST).applyTo(a)
    small = SubMap(device=0)
    small.addKeyFrame(rng.normal(size=(16, 4)).astype(np.float32), np.eye(4))
    with pytest.raises(PcrError, match="exceeds the number of key frames"):
        pg.applyTo(small)
    with pytest.raises(PcrError, match="exceeds the number of poses in the graph"):
        big = SubMap(device=0)
        for k in range(n + 1):
            big.addKeyFrame(rng.normal(size=(16, 4)).astype(np.float32), np.eye(4))
        pg.applyTo(big, 0, n + 1)
    with pytest.raises(PcrError, match="view"):
        pg.applyTo(a.view())


def test_incremental_use_matches_one_batch(references):
    """optimHandler's pattern: every key frame is added with its odometry factor and optimised; then the loops."""
    g, ref_poses, ref = references["eight-3"]
    n = len(g.poses)
    chain, loops = g.betweens[:n - 1], g.betweens[n - 1:]
    batch = gs.to_library(g, 0)
    batch.optimize(**STALL)
    inc = PoseGraph(device=0)
    inc.addPrior(g.priors[0][1], 0, g.priors[0][2])
    inc.addEstimate(0, g.poses[0])
    total = 0
    for k in range(1, n):
        # the new key frame's estimate: the previous one's current estimate moved by the odometry measurement -- what the front end hands over
        prev = inc.poses(k - 1, 1)[0]
        inc.addEstimate(k, prev @ chain[k - 1][2])
        inc.addOdomFactor(k - 1, k)
        out = inc.optimize()
        total += out.iterations
        assert out.chi2_final < 1e-12                    # a tree of factors that hold exactly: nothing to move
    again = inc.optimize()
    assert again.iterations == 0 and again.pcg_iterations == 0 and again.converged      # nothing new since the last one
    # ... then the loops, on THIS graph (add_poses + add_between_poses throughout), against one batch optimisation of a graph that holds the
    # same estimates and, as chain measurements, X_from^-1 X_to of those estimates (what add_between_poses computed, to rounding)
    est = inc.poses()
    same = gr.Graph()
    same.poses = [e.copy() for e in est]
    same.priors = list(g.priors)
    same.betweens = [(k - 1, k, gr.inv(est[k - 1]) @ est[k], gr.NOISE["odom"]) for k in range(1, n)] + list(loops)
    for i, j, Z, Om in loops:
        inc.addLC(i, j, Z, Om)
    out = inc.optimize(**STALL)
    one = gs.to_library(same, 0)
    one.optimize(**STALL)
    dt, dr = _worst(inc.poses(), one.poses())
    print(f"add_between_poses build + loops against batch: |dt| {dt:.3e} m |dR| {dr:.3e} rad; {out}")
    assert out.accepted > 0 and out.chi2_final < out.chi2_initial
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)
    # the same measurements as the batch graph's, so that both minimise the same cost
    inc2 = PoseGraph(device=0)
    inc2.addPrior(g.priors[0][1], 0, g.priors[0][2])
    inc2.addEstimate(0, g.poses[0])
    for k in range(1, n):
        inc2.addEstimate(k, g.poses[k])
        inc2.addBetween(k - 1, k, chain[k - 1][2], chain[k - 1][3])
        inc2.optimize()
    for i, j, Z, Om in loops:
        inc2.addLC(i, j, Z, Om)
    out = inc2.optimize(**STALL)
    dt, dr = _worst(inc2.poses(), batch.poses())
    print(f"incremental against batch: |dt| {dt:.3e} m |dR| {dr:.3e} rad; {out}")
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)
    dt, dr = _worst(inc2.poses(), ref_poses)
    assert dt <= BOUND_T and dr <= BOUND_R, (dt, dr)


def test_device_poses_and_apply_to_read_no_factor():
    """Factors may name poses that do not exist yet (INTEGRATION 7d adds the prior first): devicePoses and applyTo upload poses only, and
    every entry that needs the factors refuses with the message."""
    pg = PoseGraph(device=0)
    pg.addPrior(np.eye(4), 5)
    pg.addBetween(0, 2 ** 40, np.eye(4))
    X = gr.random_pose(np.random.default_rng(0), 1.0, 5.0)
    pg.addPoses(X)
    ptr, cnt = pg.devicePoses()
    assert ptr and cnt == 1
    m = SubMap(device=0)
    m.addKeyFrame(np.zeros((4, 4), np.float32), np.eye(4))
    pg.applyTo(m)
    assert np.array_equal(m.keyFrame(0)[1], X)
    for call in (pg.linearize, pg.optimize, lambda: pg.apply(0.0, np.zeros(6))):
        with pytest.raises(PcrError, match=r"prior 0: id 5 out of range"):
            call()
    # a valid graph that was never optimised
    name, g = gs.optimise_scenes()[0]
    pg = gs.to_library(g, 0)
    big = SubMap(device=0)
    for k in range(len(g.poses)):
        big.addKeyFrame(np.zeros((4, 4), np.float32), np.eye(4))
    pg.applyTo(big)
    assert all(np.array_equal(big.keyFrame(k)[1], g.poses[k]) for k in range(len(g.poses)))


def test_an_optimisation_that_did_not_converge_goes_on():
    name, g = gs.optimise_scenes()[2]
    pg = gs.to_library(g, 0)
    first = pg.optimize(max_iterations=1)
    assert first.iterations == 1 and not first.converged
    second = pg.optimize()                                  # nothing was added, but the first ran out of iterations
    assert second.iterations > 0 and second.converged and second.chi2_final < first.chi2_final
    assert second.chi2_initial == first.chi2_final
    third = pg.optimize()
    assert third.iterations == 0 and third.converged and third.chi2_final == second.chi2_final
    tighter = pg.optimize(rel_tol=1e-9, abs_tol=1e-9)       # tighter tolerances than it converged under: it goes on
    assert tighter.iterations > 0 and tighter.chi2_final <= second.chi2_final
