"""pcr_graph's robust kernels, marks and switches through the library, without a GPU (PCR_GRAPH_HOST graphs): refusals, defaults, that the
defaults change no bit, the connectivity check and the forest over the factors that are switched on, clear and g2o."""
import os
import re
import subprocess

import numpy as np
import pytest

import graph_ref as gr
import graph_robust_ref as rr
import graph_robust_scenes as rs
from simpleslam_amd import PcrError, PoseGraph
from simpleslam_amd.pcr import (ABI_SYMBOLS, GRAPH_HOST, GRAPH_ROBUST_GEMAN_MCCLURE, GRAPH_ROBUST_HUBER, GRAPH_ROBUST_NONE, GRAPH_ROBUST_TUKEY, load_library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_the_header_the_library_and_the_mirrors():
    with open(os.path.join(ROOT, "include", "pcr_hip.h")) as f:
        h = f.read()
    assert "enum { PCR_GRAPH_ROBUST_NONE = 0, PCR_GRAPH_ROBUST_HUBER = 1, PCR_GRAPH_ROBUST_GEMAN_MCCLURE = 2, PCR_GRAPH_ROBUST_TUKEY = 3 };" in h
    assert (GRAPH_ROBUST_NONE, GRAPH_ROBUST_HUBER, GRAPH_ROBUST_GEMAN_MCCLURE, GRAPH_ROBUST_TUKEY) == (0, 1, 2, 3)
    lib = load_library()
    for s in ("pcr_graph_set_robust_kernel", "pcr_graph_get_robust_kernel", "pcr_graph_set_between_robust", "pcr_graph_set_between_enabled",
              "pcr_graph_add_loop", "pcr_graph_between_weights", "pcr_graph_robust_rho_w"):
        assert re.search(r"\b" + s + r"\s*\(", h) and s in ABI_SYMBOLS and hasattr(lib, s), s
    for m in ("setRobustKernel", "setBetweenRobust", "setBetweenEnabled", "betweenWeights"):
        assert callable(getattr(PoseGraph, m)), m


def test_refusals():
    pg = rs.to_library(rs.ring12_false(), GRAPH_HOST)
    for kind in (4, -1, 99):
        with pytest.raises(PcrError, match="unknown kind"):
            pg.setRobustKernel(kind, 1.0)
    with pytest.raises(ValueError, match="unknown robust kernel"):
        pg.setRobustKernel("cauchy", 1.0)
    for kind in ("huber", "geman_mcclure", "tukey"):
        for delta in (0.0, -1.0, np.inf, -np.inf, np.nan):
            with pytest.raises(PcrError, match="delta must be finite and greater than 0"):
                pg.setRobustKernel(kind, delta)
    assert pg.robustKernel() == (GRAPH_ROBUST_NONE, 0.0)          # a refused call leaves the setting
    pg.setRobustKernel("none")                                    # NONE takes any delta
    pg.setRobustKernel("none", -3.0)
    n_between = pg.size()[2]
    assert n_between == 13
    for call in (pg.setBetweenRobust, pg.setBetweenEnabled):
        with pytest.raises(PcrError, match="exceeds the number of between factors"):
            call(n_between, 1)
        with pytest.raises(PcrError, match="exceeds the number of between factors"):
            call(5, n_between)
        call(n_between, 0)                                        # an empty range at the end is a range
    with pytest.raises(PcrError, match="exceeds the number of between factors"):
        pg.betweenWeights(1, n_between)


def test_defaults():
    g = rs.ring12_false()
    pg = rs.to_library(g, GRAPH_HOST)
    assert pg.robustKernel() == (GRAPH_ROBUST_NONE, 0.0)
    s, w, marked, on = pg.betweenWeights()
    assert on.all() and (w == 1.0).all() and s.shape == (13,)
    assert list(marked) == [False] * 11 + [True, True]            # addBetween does not mark, addLC does
    pg.setBetweenRobust(2, 3)
    pg.setBetweenRobust(12, 1, False)
    assert list(pg.betweenWeights()[2]) == [False, False, True, True, True] + [False] * 6 + [True, False]
    pg.setRobustKernel("tukey", 0.5)
    assert pg.robustKernel() == (GRAPH_ROBUST_TUKEY, 0.5)
    # every output pointer may be NULL
    assert load_library().pcr_graph_between_weights(pg._g, 0, 13, None, None, None, None) == 0


def test_marks_change_no_bit_under_the_defaults():
    g = rs.ring12()
    a, b = rs.to_library(g, GRAPH_HOST), rs.to_library(g, GRAPH_HOST, marks=False)
    assert a.betweenWeights()[2].any() and not b.betweenWeights()[2].any()
    la, lb = a.linearize(), b.linearize()
    for x, y in zip(la[:3], lb[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.float64(la[3]).view(np.uint64) == np.float64(lb[3]).view(np.uint64)
    wa, wb = a.betweenWeights(), b.betweenWeights()
    assert np.array_equal(_bits(wa[0]), _bits(wb[0])) and np.array_equal(wa[1], wb[1]) and (wa[1] == 1.0).all()
    # chi2 is the plain sum it was: the fold of s over priors and between factors
    r, _, _, chi2 = la
    want = r[0] @ gr.NOISE["prior"] @ r[0] + wa[0].sum()
    assert abs(chi2 - want) <= 1e-12 * chi2


def _chain4():
    """0 - 1 - 2 - 3, a prior on 0, and a loop 0 -> 2 that duplicates the path over pose 1"""
    g = rr.RobustGraph()
    g.poses = [gr.exp(np.array([0, 0, 0.1 * k, 1.0 * k, 0, 0])) for k in range(4)]
    g.priors.append((0, g.poses[0], gr.NOISE["prior"]))
    for i in range(3):
        g.add_between(i, i + 1, gr.inv(g.poses[i]) @ g.poses[i + 1], gr.NOISE["odom"])
    g.add_loop(0, 2, gr.inv(g.poses[0]) @ g.poses[2], gr.NOISE["loop"])
    return g


def test_disabling_the_only_edge_to_a_pose_is_refused_and_named():
    pg = rs.to_library(_chain4(), GRAPH_HOST)
    assert pg.tree()[1:] == (3, 1)
    pg.setBetweenEnabled(2, 1, False)                             # 2 -> 3: pose 3 loses its only link
    with pytest.raises(PcrError, match=r"pcr_graph_tree: pose 3 lies in a connected component without a prior"):
        pg.tree()
    with pytest.raises(PcrError, match=r"pcr_graph_optimize: pose 3 lies in a connected component without a prior"):
        pg.optimize()
    assert pg.size() == (4, 1, 4)                                 # it stays in the graph
    pg.linearize()                                                # ... and linearises: r and J of every factor
    pg.setBetweenEnabled(2, 1, True)
    parent, n_tree, n_other = pg.tree()
    assert (list(parent), n_tree, n_other) == ([-1, 0, 1, 2], 3, 1)


def test_a_loop_replaces_a_disabled_forest_edge():
    pg = rs.to_library(_chain4(), GRAPH_HOST)
    parent, n_tree, n_other = pg.tree()
    assert (list(parent), n_tree, n_other) == ([-1, 0, 1, 2], 3, 1)
    pg.setBetweenEnabled(0, 1, False)                             # 0 -> 1: the loop 0 -> 2 now links {1, 2, 3} to the prior
    parent, n_tree, n_other = pg.tree()
    assert (list(parent), n_tree, n_other) == ([-1, 2, 0, 2], 3, 0)
    pg.setBetweenEnabled(3, 1, False)                             # ... and without it nothing does
    with pytest.raises(PcrError, match=r"pose 1 lies in a connected component without a prior"):
        pg.tree()
    pg.setBetweenEnabled(0, 1, True)
    parent, n_tree, n_other = pg.tree()
    assert (list(parent), n_tree, n_other) == ([-1, 0, 1, 2], 3, 0)          # the loop is off: it is in neither count


def test_clear_resets_marks_and_switches_and_keeps_the_kernel():
    g = _chain4()
    pg = rs.to_library(g, GRAPH_HOST)
    pg.setRobustKernel("huber", 0.7)
    pg.setBetweenEnabled(3, 1, False)
    pg.setBetweenRobust(0, 2)
    pg.clear()
    assert pg.size() == (0, 0, 0) and pg.robustKernel() == (GRAPH_ROBUST_HUBER, 0.7)
    pg.addPoses(np.stack(g.poses))
    pg.addPrior(g.priors[0][1], 0, g.priors[0][2])
    for i, j, Z, Om in g.betweens:
        pg.addBetween(i, j, Z, Om)
    _, w, marked, on = pg.betweenWeights()
    assert not marked.any() and on.all() and (w == 1.0).all()


def test_g2o_carries_every_factor_and_no_mark(tmp_path):
    g = rs.ring12_false()
    pg = rs.to_library(g, GRAPH_HOST)
    pg.setBetweenEnabled(12, 1, False)
    path = str(tmp_path / "ring.g2o")
    pg.saveG2o(path)
    with open(path) as f:
        assert sum(1 for line in f if line.startswith("EDGE_SE3:QUAT")) == 13          # the one that is off is written too
    back = PoseGraph(device=GRAPH_HOST)
    back.loadG2o(path)
    assert back.size() == (12, 1, 13)
    s, w, marked, on = back.betweenWeights()
    assert not marked.any() and on.all()
    assert np.abs(s - pg.betweenWeights()[0]).max() <= 1e-9 * s.max()          # the same factors, through 17 digits and a quaternion


CPP = r'''
#include "PCR/HipRegister.hpp"
double run(backend::PoseGraph& g, const PCR::pose_t& z) {
    g.addLC(3, 9, z);
    g.setRobustKernel(PCR_GRAPH_ROBUST_TUKEY, 0.1);
    g.setBetweenRobust(0, 2, false);
    backend::PoseGraph::Result r = g.optimize();
    backend::PoseGraph::Weights v = g.betweenWeights();
    for (size_t e = 0; e < v.w.size(); ++e) if (v.robust[e] && v.w[e] < 0.01) g.setBetweenEnabled(e, 1, false);
    r = g.optimize();
    return r.chi2_final + v.s[0] + (double)v.enabled.size() + g.betweenWeights(1, 2).w[0];
}
'''


def test_the_cpp_mirror_compiles(tmp_path):
    (tmp_path / "use.cpp").write_text(CPP)
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "simpleslam_amd", "host"), str(tmp_path / "use.cpp")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
