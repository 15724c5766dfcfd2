"""The tree preconditioner's spanning forest without a device: pcr_graph_tree on PCR_GRAPH_HOST graphs against the rule
restated in graph_tree_ref, its refusals, the new parameter's default and range, the mirrors, and the stand-alone check of the plan's
invariants (host/graph_forest_check.cpp) over the scenes' edge lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_scenes as gs
import graph_tree_ref as tr
import graph_tree_scenes as ts
from simpleslam_amd import PcrError, PoseGraph
from simpleslam_amd.pcr import (ABI_SYMBOLS, GRAPH_HOST, GRAPH_PRECOND_BLOCK_JACOBI, GRAPH_PRECOND_TREE, GraphParams, load_library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ts.NAMES)
def test_the_forest_is_the_restated_rule(name):
    g = ts.scenes()[name]
    want = tr.graph_forest(g)
    parent, n_tree, n_other = gs.to_library(g, GRAPH_HOST).tree()
    assert parent.dtype == np.int64 and parent.shape == (len(g.poses),)
    assert np.array_equal(parent, want["parent"]), np.flatnonzero(parent != want["parent"])[:8]
    assert (n_tree, n_other) == (want["n_tree"], want["n_other"])
    assert n_tree + n_other == len(g.betweens)
    # roots: one per component, each the lowest-numbered pose of its component that holds a prior
    roots = set(np.flatnonzero(parent < 0).tolist())
    assert len(roots) == len(g.poses) - n_tree
    held = sorted(k for k, _, _ in g.priors)
    assert roots <= set(held)


def test_the_scenes_are_the_shapes_they_claim():
    s = ts.scenes()
    f = {n: tr.graph_forest(s[n]) for n in ts.NAMES}
    assert f["n1"]["n_tree"] == 0 and f["n2"]["n_tree"] == 1
    p = f["reversed-chain"]["parent"]
    assert all(p[k] == k + 1 for k in range(len(p) - 1)) and p[-1] == -1            # every parent id > its child's
    assert (f["star"]["parent"][1:] == 0).all() and f["star"]["n_other"] == 3
    t = s["tree200"]
    assert f["tree200"]["n_other"] == 4 and any(i > j for i, j, _, _ in t.betweens[199:])
    assert sum(1 for i, j, _, _ in t.betweens if (i, j) == t.betweens[199 + 2][:2]) == 2      # the duplicate of a tree edge
    assert sorted(np.flatnonzero(f["two-components"]["parent"] < 0)) == [0, 17]
    assert len(s["inner-prior"].priors) == 2 and (f["inner-prior"]["parent"] < 0).sum() == 1
    assert len(s["chain1025"].poses) == 1025 and f["chain1025"]["n_other"] == 1


def test_a_duplicate_and_a_backward_edge_are_loops_whatever_their_noise():
    pg = PoseGraph(device=GRAPH_HOST)
    pg.addPoses(np.stack([np.eye(4)] * 4))
    pg.addPrior(np.eye(4), 2)
    for i, j in ((1, 0), (1, 0), (2, 1), (0, 2), (3, 2)):        # the second is a duplicate, the fourth closes 0-1-2
        pg.addBetween(i, j, np.eye(4))
    parent, n_tree, n_other = pg.tree()
    assert parent.tolist() == [1, 2, -1, 2] and (n_tree, n_other) == (3, 2)


def test_the_forest_follows_the_graph_as_it_grows():
    pg = PoseGraph(device=GRAPH_HOST)
    pg.addPoses(np.stack([np.eye(4)] * 2))
    pg.addPrior(np.eye(4))
    pg.addBetween(0, 1, np.eye(4))
    assert pg.tree()[0].tolist() == [-1, 0]
    assert pg.tree()[0].tolist() == [-1, 0]          # nothing was added: the same forest
    pg.addPoses(np.eye(4))
    pg.addBetween(2, 0, np.eye(4))
    assert pg.tree() [0].tolist() == [-1, 0, 0]
    pg.addLC(1, 2, np.eye(4))
    parent, n_tree, n_other = pg.tree()
    assert parent.tolist() == [-1, 0, 0] and (n_tree, n_other) == (2, 1)
    pg.clear()
    assert pg.tree()[0].size == 0


def _four():
    pg = PoseGraph(device=GRAPH_HOST)
    pg.addPoses(np.stack([np.eye(4)] * 4))
    pg.addPrior(np.eye(4))
    for i in range(3):
        pg.addBetween(i, i + 1, np.eye(4))
    return pg


def test_tree_refuses_what_optimize_refuses():
    bad = np.eye(4)
    bad[1, 3] = np.nan
    info = np.eye(6)
    info[2, 4] = info[4, 2] = np.inf
    cases = [
        (lambda pg: pg.addBetween(2, 2, np.eye(4)), r"between factor 3: from == to \(2\)"),
        (lambda pg: pg.addBetween(1, 9, np.eye(4)), r"between factor 3: id 9 out of range \(the graph holds 4 poses\)"),
        (lambda pg: pg.addPrior(np.eye(4), 4), r"prior 1: id 4 out of range"),
        (lambda pg: (pg.addPoses(bad), pg.addBetween(3, 4, np.eye(4))), r"pose 4 is not finite"),
        (lambda pg: pg.addBetween(0, 3, np.eye(4), info), r"between factor 3: the information matrix is not finite"),
        (lambda pg: pg.addBetween(0, 3, bad), r"between factor 3: the pose is not finite"),
        (lambda pg: pg.addPoses(np.eye(4)), r"pose 4 lies in a connected component without a prior"),
    ]
    for spoil, msg in cases:
        for call in ("tree", "optimize"):
            pg = _four()
            spoil(pg)
            with pytest.raises(PcrError, match=msg):
                getattr(pg, call)()
    pg = PoseGraph(device=GRAPH_HOST)
    pg.addPrior(np.eye(4), 5)
    pg.addBetween(0, 2 ** 40, np.eye(4))
    pg.addPoses(np.eye(4))
    with pytest.raises(PcrError, match=r"prior 0: id 5 out of range \(the graph holds 1 poses\)"):
        pg.tree()
    assert PoseGraph(device=GRAPH_HOST).tree()[1:] == (0, 0)          # an empty graph has an empty forest


def test_tree_checks_the_room_it_is_given():
    pg = _four()
    lib = load_library()
    parent = np.zeros(3, dtype=np.int64)
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert lib.pcr_graph_tree(pg._g, parent.ctypes.data_as(C.POINTER(C.c_int64)), 3, C.byref(a), C.byref(b)) != 0
    assert b"room for 3" in lib.pcr_graph_last_error(pg._g)
    assert lib.pcr_graph_tree(pg._g, None, 0, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (3, 0)      # the counts alone


def test_the_default_is_block_jacobi_and_an_unknown_value_is_refused():
    p = GraphParams()
    load_library().pcr_graph_default_params(C.byref(p))
    assert p.struct_size == C.sizeof(GraphParams) == 72
    assert p.pcg_preconditioner == GRAPH_PRECOND_BLOCK_JACOBI == 0 and GRAPH_PRECOND_TREE == 1
    for bad in (2, -1, 7):
        with pytest.raises(PcrError, match=r"unknown pcg_preconditioner %d" % bad):
            _four().optimize(pcg_preconditioner=bad)
    with pytest.raises(ValueError, match="unknown preconditioner"):
        _four().optimize(pcg_preconditioner="jacobi")
    for ok in ("tree", "block_jacobi", GRAPH_PRECOND_TREE, GRAPH_PRECOND_BLOCK_JACOBI):
        with pytest.raises(PcrError, match=r"PCR_GRAPH_HOST graph has no device"):          # known: the next refusal is the host graph's
            _four().optimize(pcg_preconditioner=ok)
    with pytest.raises(PcrError, match=r"PCR_GRAPH_HOST graph has no device"):
        _four().precondition(0.0, np.zeros(24), "tree")
    with pytest.raises(PcrError, match=r"unknown preconditioner 5"):
        _four().precondition(0.0, np.zeros(24), 5)


def test_the_header_the_library_and_the_mirrors():
    with open(os.path.join(ROOT, "include", "pcr_hip.h")) as f:
        h = f.read()
    assert "enum { PCR_GRAPH_PRECOND_BLOCK_JACOBI = 0, PCR_GRAPH_PRECOND_TREE = 1 };" in h
    assert re.search(r"pcg_rel_tol;[^}]*int32_t pcg_preconditioner;[^}]*\} pcr_graph_params;", h, re.S)          # appended: the last field
    lib = load_library()
    for s in ("pcr_graph_tree", "pcr_graph_precondition"):
        assert re.search(r"\b" + s + r"\s*\(", h) and s in ABI_SYMBOLS and hasattr(lib, s), s
    assert callable(PoseGraph.tree) and callable(PoseGraph.precondition)


CPP = r'''
#include "PCR/HipRegister.hpp"
double run(backend::PoseGraph& g) {
    size_t n_tree = 0, n_other = 0;
    std::vector<int64_t> parent = g.tree(&n_tree, &n_other);
    std::vector<double> z = g.precondition(1e-5, std::vector<double>(6 * g.poses(), 1.0), PCR_GRAPH_PRECOND_TREE);
    backend::PoseGraph::Result r = g.optimize(PCR_GRAPH_PRECOND_TREE);
    pcr_graph_params p;
    pcr_graph_default_params(&p);
    p.pcg_preconditioner = PCR_GRAPH_PRECOND_BLOCK_JACOBI;
    r = g.optimize(&p);
    return z[0] + (double)parent.size() + r.chi2_final;
}
'''


def test_the_cpp_mirror_compiles(tmp_path):
    (tmp_path / "use.cpp").write_text(CPP)
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "simpleslam_amd", "host"), str(tmp_path / "use.cpp")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_plans_invariants_hold_on_every_scene(tmp_path):
    """host/graph_forest_check.cpp plans each edge list with csrc/graph_forest.h and checks the schedule: positions are an elimination order,
    paths follow the heavy children, every path's round is 1 + the largest round hanging off it, at most log2(N) + 1 rounds."""
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "graph_forest_check")
    assert os.path.exists(exe), "build() makes it (csrc/Makefile: harness)"
    lines = []
    for name in ts.NAMES:
        g = ts.scenes()[name]
        lines.append(f"graph {name} {len(g.poses)}")
        lines += [f"prior {k}" for k, _, _ in g.priors] + [f"edge {i} {j}" for i, j, _, _ in g.betweens]
    path = tmp_path / "edges.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {line.split(":")[0]: line for line in out.stdout.splitlines() if ":" in line}
    assert set(rows) == set(ts.NAMES)
    assert rows["chain300"].endswith("roots 1 paths 1 rounds 1")                    # a chain is one path in round 0
    assert rows["star"].endswith("roots 1 paths 64 rounds 2")                       # 63 leaves in round 0; the hub, with leaf 1 below it, in round 1
    assert "roots 2" in rows["two-components"]
    assert out.stdout.splitlines()[-1] == f"{len(ts.NAMES)} graphs, 0 failed"
    own = subprocess.run([exe], capture_output=True, text=True, timeout=120)            # its built-in set, a 20 000-pose chain among it
    assert own.returncode == 0, own.stdout + own.stderr
