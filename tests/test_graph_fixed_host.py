"""Fixed poses through the library without a GPU (PCR_GRAPH_HOST graphs, DESIGN.md 4.17 "Fixed poses"): the defaults, the refusals and that
each leaves the store untouched, the anchor rule of the connectivity check, the forest's root rule, FIX records in g2o files, and that the
flags change no bit of a host linearisation.  (That set-then-clear counts as something new for pcr_graph_optimize needs a device graph:
test_graph_fixed_gpu.py; the store's revision counter itself is worked in host/graph_host_check.cpp.)"""
import os
import re

import numpy as np
import pytest

import graph_fixed_scenes as fs
import graph_scenes as gs
from simpleslam_amd import PcrError, PoseGraph
from simpleslam_amd.pcr import ABI_SYMBOLS, GRAPH_HOST, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_small.g2o")
NO_PRIOR = r"pose {} lies in a connected component without a prior: the system would be singular"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _chain(n, prior=None):
    """n identity poses in a chain 0 - 1 - ... - n-1, a prior on `prior` when given"""
    pg = PoseGraph(device=GRAPH_HOST)
    pg.addPoses(np.stack([np.eye(4)] * n))
    if prior is not None:
        pg.addPrior(np.eye(4), prior)
    for k in range(1, n):
        pg.addBetween(k - 1, k, np.eye(4))
    return pg


def test_the_header_the_library_and_the_mirrors():
    with open(os.path.join(ROOT, "include", "pcr_hip.h")) as f:
        h = f.read()
    lib = load_library()
    for s in ("pcr_graph_set_fixed", "pcr_graph_fixed"):
        assert re.search(r"\b" + s + r"\s*\(", h) and s in ABI_SYMBOLS and hasattr(lib, s), s
    assert "int pcr_graph_set_fixed(pcr_graph* g, size_t first, size_t count, int on);" in h
    assert "int pcr_graph_fixed(const pcr_graph* g, size_t first, size_t count, uint8_t* fixed);" in h
    for m in ("setFixed", "fixed"):
        assert callable(getattr(PoseGraph, m)), m
    with open(os.path.join(ROOT, "simpleslam_amd", "host", "PCR", "HipRegister.hpp")) as f:
        hpp = f.read()
    assert "void setFixed(size_t first, size_t count = 1, bool on = true)" in hpp and "fixed() const" in hpp


def test_nothing_is_fixed_by_default():
    pg = gs.to_library(fs.scenes()["chain12"], GRAPH_HOST)
    assert pg.fixed().dtype == bool and pg.fixed().shape == (12,) and not pg.fixed().any()
    assert PoseGraph(device=GRAPH_HOST).fixed().shape == (0,)
    golden = PoseGraph(device=GRAPH_HOST)
    golden.loadG2o(GOLDEN)                                  # a file without FIX records fixes nothing
    assert golden.fixed().size == golden.size()[0] > 0 and not golden.fixed().any()
    pg.setFixed(3)                                          # count = 1, on = True
    pg.setFixed(6, 2)
    assert np.flatnonzero(pg.fixed()).tolist() == [3, 6, 7]
    pg.setFixed(6, 1, False)
    assert np.flatnonzero(pg.fixed()).tolist() == [3, 7]
    pg.addPoses(np.eye(4))                                  # a new pose is free, the flags stay with their poses
    assert np.flatnonzero(pg.fixed()).tolist() == [3, 7] and pg.fixed().size == pg.size()[0]
    pg.clear()                                              # clear resets the flags as it resets marks and switches
    pg.addPoses(np.stack([np.eye(4)] * 8))
    assert not pg.fixed().any()


def test_a_range_beyond_the_poses_is_refused_and_leaves_the_store(tmp_path):
    pg = fs.to_library(fs.scenes()["chain12"], GRAPH_HOST)
    before = str(tmp_path / "before.g2o")
    pg.saveG2o(before)
    fixed, lin = pg.fixed().copy(), pg.linearize()
    for first, count in ((12, 1), (13, 0), (0, 13), (5, 8), (11, 2 ** 63)):
        for on in (True, False):
            with pytest.raises(PcrError, match=r"pcr_graph_set_fixed: first \+ count exceeds the number of poses \(12\)"):
                pg.setFixed(first, count, on)
    with pytest.raises(PcrError, match="must not be negative"):
        pg.setFixed(-1)
    pg.setFixed(12, 0)                                      # an empty range at the end is a range
    assert np.array_equal(pg.fixed(), fixed) and fixed.sum() == 4
    after = str(tmp_path / "after.g2o")
    pg.saveG2o(after)
    assert open(before, "rb").read() == open(after, "rb").read()
    for a, b in zip(lin, pg.linearize()):
        assert np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))
    lib = load_library()
    import ctypes as C
    assert lib.pcr_graph_fixed(pg._g, 5, 8, None) != 0 and b"pcr_graph_fixed: first + count exceeds the number of poses (12)" in lib.pcr_graph_last_error(pg._g)
    assert lib.pcr_graph_fixed(pg._g, 0, 12, None) != 0 and b"NULL output" in lib.pcr_graph_last_error(pg._g)
    two = (C.c_uint8 * 2)(9, 9)
    assert lib.pcr_graph_fixed(pg._g, 7, 2, two) == 0 and list(two) == [1, 0]


def test_a_fix_record_of_an_unknown_id_is_refused_and_leaves_the_store(tmp_path):
    pg = _chain(4, prior=0)
    pg.setFixed(1)
    v4 = "VERTEX_SE3:QUAT 4 1 2 3 0 0 0 1\n"
    for text, msg in ((v4 + "FIX 5\n", r":2: FIX 5: the file defines no vertex of that id"),
                      (v4 + "FIX 1\n", r":2: FIX 1: the file defines no vertex of that id"),          # the graph's own pose, not the file's
                      ("FIX 4 6\n" + v4, r":1: FIX 6: the file defines no vertex of that id"),
                      (v4 + "FIX -2\n", r":2: FIX -2: the file defines no vertex of that id"),
                      (v4 + "FIX\n", r":2: malformed FIX")):
        path = tmp_path / "bad.g2o"
        path.write_text(text)
        with pytest.raises(PcrError, match=msg):
            pg.loadG2o(str(path))
        assert pg.size() == (4, 1, 3) and pg.fixed().tolist() == [False, True, False, False]
    path.write_text("FIX 4\n" + v4 + "VERTEX_SE3:QUAT 5 0 0 0 0 0 0 1\nFIX 5 4\n")      # before its vertex, twice, several ids on a line
    pg.loadG2o(str(path))
    assert pg.size() == (6, 1, 3) and pg.fixed().tolist() == [False, True, False, False, True, True]


def test_a_fixed_pose_anchors_its_component():
    pg = _chain(5)                                          # no prior anywhere
    with pytest.raises(PcrError, match=NO_PRIOR.format(0)):
        pg.tree()
    pg.setFixed(3)
    parent, n_tree, n_other = pg.tree()                     # accepted: the fixed pose is the only anchor, and the root
    assert parent.tolist() == [1, 2, 3, -1, 3] and (n_tree, n_other) == (4, 0)
    pg.setBetweenEnabled(1, 1, False)                       # 1 - 2 off: {0, 1} loses the edge that joins it to its fixed pose
    with pytest.raises(PcrError, match=r"pcr_graph_tree: " + NO_PRIOR.format(0)):
        pg.tree()
    pg.setBetweenEnabled(1, 1, True)
    pg.setBetweenEnabled(3, 1, False)                       # 3 - 4 off: pose 4 is named
    with pytest.raises(PcrError, match=NO_PRIOR.format(4)):
        pg.tree()
    pg.setFixed(4)                                          # ... until it is fixed itself: a lone fixed pose is anchored
    assert pg.tree()[0].tolist() == [1, 2, 3, -1, -1]
    pg.setFixed(0, 5, False)
    with pytest.raises(PcrError, match=NO_PRIOR.format(0)):
        pg.tree()
    with pytest.raises(PcrError, match=r"pcr_graph_optimize: " + NO_PRIOR.format(0)):
        pg.optimize()
    pg.setFixed(2)
    pg.setBetweenEnabled(3, 1, True)
    with pytest.raises(PcrError, match="PCR_GRAPH_HOST graph has no device"):      # the graph itself is accepted: the next refusal in order
        pg.optimize()


def test_the_prior_only_cases_behave_as_before():
    pg = _chain(5, prior=0)
    assert pg.tree()[0].tolist() == [-1, 0, 1, 2, 3]
    pg.setBetweenEnabled(2, 1, False)
    with pytest.raises(PcrError, match=NO_PRIOR.format(3)):
        pg.tree()
    pg.setBetweenEnabled(2, 1, True)
    pg.setFixed(0, 5)
    pg.setFixed(0, 5, False)                                # flags set and cleared: the prior-only rule again
    assert pg.tree()[0].tolist() == [-1, 0, 1, 2, 3]
    pg.setBetweenEnabled(2, 1, False)
    with pytest.raises(PcrError, match=NO_PRIOR.format(3)):
        pg.tree()


def test_the_root_is_the_lowest_numbered_anchor():
    pg = _chain(12, prior=8)
    assert pg.tree()[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, -1, 8, 9, 10]                    # no flag: the prior's pose, as ever
    pg.setFixed(4, 4)
    assert pg.tree()[0].tolist() == [1, 2, 3, 4, -1, 4, 5, 6, 7, 8, 9, 10]                    # 4 < 8: a fixed root with children on both sides
    pg.setFixed(4, 4, False)
    pg.setFixed(10)
    assert pg.tree()[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, -1, 8, 9, 10]                    # 8 < 10: the prior's pose stays the root
    for name in fs.NAMES:                                                                      # the scenes, without and with their flags
        g = fs.scenes()[name]
        anchors = sorted(set(k for k, _, _ in g.priors) | g.fixed)
        parent = fs.to_library(g, GRAPH_HOST).tree()[0]
        assert np.flatnonzero(parent < 0).tolist() == [anchors[0]], name
        if g.priors:
            free = fs.to_library(g, GRAPH_HOST, fixed=False)
            assert np.array_equal(free.tree()[0], gs.to_library(g, GRAPH_HOST).tree()[0])


def _exact_graph():
    """Six poses and seven between factors whose rotations are the identity, half turns about the axes and the third of a turn about
    (1, 1, 1) -- quaternions of entries 0, 1/2 and 1 -- with dyadic translations: the writer's quaternion of such a pose and the reader's
    matrix of that quaternion are both exact, so a second save repeats the first one's text.  (For a general rotation the last digit of a
    quaternion entry may differ between the two saves, with flags or without: test_graph_host.py's round trip allows 1e-14 for that.  It
    is the writer's conversion, not the flags, and is kept out of this comparison.)  The information matrices are full and arbitrary: 17
    digits carry their bits."""
    rots = [np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]),
            np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])]
    rng = np.random.default_rng(81)
    pg = PoseGraph(device=GRAPH_HOST)

    def pose(k):
        T = np.eye(4)
        T[:3, :3] = rots[k % 6]
        T[:3, 3] = (0.5 * k, -1.25 * k, 3.0 - 0.125 * k)
        return T
    pg.addPoses(np.stack([pose(k) for k in range(6)]))
    pg.addPrior(pose(0), 0)
    for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (2, 4))):
        pg.addBetween(i, j, pose(e + 2), gs.full_info(rng))
    return pg


def test_g2o_round_trip_with_flags(tmp_path):
    a = _exact_graph()
    n = a.size()[0]
    plain = str(tmp_path / "plain.g2o")
    a.saveG2o(plain)
    assert b"FIX" not in open(plain, "rb").read()
    a.setFixed(0, 2)
    a.setFixed(n - 1)
    one, two = str(tmp_path / "one.g2o"), str(tmp_path / "two.g2o")
    a.saveG2o(one)
    lines = open(one).read().splitlines()
    tags = [line.split()[0] for line in lines]
    assert tags == ["VERTEX_SE3:QUAT"] * n + ["FIX"] * 3 + ["EDGE_SE3:QUAT"] * a.size()[2]   # one record per fixed pose, after the vertices
    assert lines[n:n + 3] == ["FIX 0", "FIX 1", f"FIX {n - 1}"]
    assert [l for l in lines if not l.startswith("FIX")] == open(plain).read().splitlines()    # and nothing else moves
    b = PoseGraph(device=GRAPH_HOST)
    b.loadG2o(one)
    assert np.array_equal(a.fixed(), b.fixed()) and a.size() == b.size()
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    b.saveG2o(two)
    assert open(one, "rb").read() == open(two, "rb").read()                                   # save, load, save: identical bytes
    # a save without flags equals a save from a graph never given the new calls
    a.setFixed(0, n, False)
    cleared = str(tmp_path / "cleared.g2o")
    a.saveG2o(cleared)
    assert open(cleared, "rb").read() == open(plain, "rb").read()
    # the golden file, whose rotations are general: the records and their order survive the round trip
    g = PoseGraph(device=GRAPH_HOST)
    g.loadG2o(GOLDEN)
    g.setFixed(2, 3)
    g.saveG2o(one)
    h = PoseGraph(device=GRAPH_HOST)
    h.loadG2o(one)
    h.saveG2o(two)
    tags_of = lambda path: [l.split()[0] if not l.startswith("FIX") else l for l in open(path).read().splitlines()]
    assert tags_of(one) == tags_of(two) and tags_of(one).count("FIX 3") == 1 and np.flatnonzero(h.fixed()).tolist() == [2, 3, 4]


@pytest.mark.parametrize("name", fs.NAMES)
def test_the_flags_change_no_bit_of_a_host_linearisation(name):
    g = fs.scenes()[name]
    free, held = fs.to_library(g, GRAPH_HOST, fixed=False), fs.to_library(g, GRAPH_HOST)
    assert held.fixed().sum() == len(g.fixed) and not free.fixed().any()
    want = free.linearize()
    for what, a, b in zip(("r", "J_from", "J_to", "chi2"), want, held.linearize()):
        assert np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b))), (name, what)     # unweighted r and J for every factor, chi2 over all
    assert abs(want[3] - g.chi2()) <= 1e-11 * want[3]
    for what, a, b in zip(("s", "w"), free.betweenWeights()[:2], held.betweenWeights()[:2]):
        assert np.array_equal(_bits(a), _bits(b)), (name, what)
    held.setFixed(0, len(g.poses), False)                                                    # set then clear: the next linearisation is bit-identical
    for what, a, b in zip(("r", "J_from", "J_to", "chi2"), want, held.linearize()):
        assert np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b))), (name, what)
