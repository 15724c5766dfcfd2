"""Scenes of the fixed-pose tests: name -> graph_fixed_ref.FixedGraph, built once (scenes()).  The smallest shapes at which the kernels can
still go wrong with fixed poses: a graph whose only anchor is a fixed pose, a fixed block inside a chain (the forest then has fixed interior
nodes with children on both sides), loops that cross the boundary between fixed and free, and more factors than one wave (64) and one
block (256) of the linearise grid with fixed ids at the wave edge (63, 64) and at the end."""
import functools

import numpy as np

import graph_fixed_ref as fr
import graph_ref as gr
import graph_robust_scenes as rs
import graph_scenes as gs
import graph_tree_scenes as ts


def chain6():
    """a 6-pose chain with one loop 5 -> 0, NO prior: pose 0 is fixed and is all that holds the graph"""
    rng = np.random.default_rng(61)
    truth = ts._walk(rng, 6, lambda k: k - 1)
    edges = [(k - 1, k, "odom") for k in range(1, 6)] + [(5, 0, "loop")]
    g = ts.build(truth, edges, [], 62)
    return fr.FixedGraph.of(g, [0])


def chain12():
    """a 12-pose chain with two loops and a prior on 0; poses 4 .. 7, a block in the middle, are fixed"""
    rng = np.random.default_rng(63)
    truth = ts._walk(rng, 12, lambda k: k - 1)
    edges = [(k - 1, k, "odom") for k in range(1, 12)] + [(11, 0, "loop"), (2, 9, "loop")]
    g = ts.build(truth, edges, [0], 64)
    return fr.FixedGraph.of(g, range(4, 8))


def eight41():
    """the figure of eight over 41 poses with three loops at its crossing (0, 20, 40); the first half (0 .. 19) is fixed, so that two loops
    and the chain edge 19 -> 20 cross the boundary"""
    g = gs.loop_graph(gs.eight_truth(41), [(0, 40), (0, 20), (20, 40)], 65)
    return fr.FixedGraph.of(g, range(20))


G70_FIXED = (0, 7, 8, 31, 63, 64, 69)


def g70():
    """70 poses, every pose tied to the ones 1, 2, 3 and 5 before it: 270 factors with the prior, so that they span five waves and two blocks
    of the linearise grid.  The fixed ids are scattered and include 63, 64 and the last pose."""
    rng = np.random.default_rng(67)
    truth = ts._walk(rng, 70, lambda k: k - 1)
    edges = [(k - 1, k, "odom") for k in range(1, 70)]
    for step in (2, 3, 5):
        edges += [(k - step, k, "loop") for k in range(step, 70)]
    g = ts.build(truth, edges, [0], 68)
    assert len(g.priors) + len(g.betweens) == 270
    return fr.FixedGraph.of(g, G70_FIXED)


def ring12_false_into_fixed():
    """graph_robust_scenes.ring12_false with pose 9 fixed: the false loop 3 -> 9 ends in a fixed pose"""
    return fr.FixedGraph.of(rs.ring12_false(), [rs.FALSE_LOOP[1]])


NAMES = ("chain6", "chain12", "eight41", "g70")


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> graph; built once and never modified (copy() before optimising)"""
    return {"chain6": chain6(), "chain12": chain12(), "eight41": eight41(), "g70": g70()}


def to_library(g, device, fixed=True, kind=None):
    """a PoseGraph holding FixedGraph g (graph_robust_scenes.to_library), then its fixed flags in runs of consecutive ids (fixed=False: none)"""
    pg = rs.to_library(g, device, kind=kind)
    if fixed:
        ids = sorted(g.fixed)
        k = 0
        while k < len(ids):
            n = 1
            while k + n < len(ids) and ids[k + n] == ids[k] + n:
                n += 1
            pg.setFixed(ids[k], n)
            k += n
    return pg
