"""The body of a LOAM Gauss-Newton launch -- posting of the cache misses by wave ballot, the chunk sums of the normal equations, the store of
the cache entries -- at the smallest shapes that reach each of its branches.

What is compared is exact: the miss exchange decides WHO searches a query, never what the search returns, so a call with the neighbour cache must
give the pose, the per-launch sums and the steps of the same call on a handle without it (loam_disable_cache = 1), bit for bit.  Single-block scans
make a launch's `searches` in the trace the block's miss count, which selects the route: 0 none, 1-8 one wave per query, 9-64 four lanes per query,
65-128 two lanes per query, 129-256 every lane its own query."""
import functools

import numpy as np
import pytest

import oracle
from simpleslam_amd import LoamRegister, pcr, synth

pytestmark = pytest.mark.gpu

SEED = 7
ITERS = 6
# initial perturbation (metres, degrees), from what a first guess is off by down to what the last Gauss-Newton steps move
# (the last two sit just under the step size at which a launch gives up its cache entries altogether: launches that miss in part)
LADDER = ((0.3, 2.0), (0.1, 1.0), (0.03, 0.3), (0.01, 0.1), (0.003, 0.03), (0.001, 0.01), (0.045, 0.4), (0.06, 0.5))
SINGLE_BLOCK = (256, 200, 65, 64, 1)
MULTI_BLOCK = (257, 513, 700)
CLASSES = ((0, 0), (1, 8), (9, 64), (65, 128), (129, 255), (256, 256))
# (n_src, rung of LADDER) of test_few_writers_leave_whole_entries: a call with a launch of 1-8 searches behind launch 0
FEW_WRITER_CASE = (256, 2)


@functools.lru_cache(maxsize=None)
def _world():
    world, m = synth.make_map(20_000, seed=SEED)
    scan, T = synth.make_scan(world, 0, seed=SEED, beams=16, azimuths=128)
    for v in (m, scan, T):
        v.setflags(write=False)
    return m, scan, T


@functools.lru_cache(maxsize=None)
def _scan(n_src):
    _, scan, _ = _world()
    s = np.ascontiguousarray(scan[np.linspace(0, len(scan) - 1, n_src).astype(int)])      # spread over the whole sweep
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _init(rung):
    _, _, T = _world()
    trans, rot = LADDER[rung]
    T0 = synth.perturb(T, SEED + rung, trans=trans, rot_deg=rot)
    T0.setflags(write=False)
    return T0


def _call(reg, n_src, rung):
    m, _, _ = _world()
    pose = _init(rung).copy()
    conv = reg.scan2Map(_scan(n_src), m, pose)
    return pose, conv, reg.trace()


@functools.lru_cache(maxsize=None)
def _pair(n_src, rung, coresident=0):
    """(cached, uncached) results of one call: computed once, shared by the tests below."""
    out = []
    for disable in (0, 1):
        prm = pcr.default_params(loam_iters=ITERS, loam_early_exit=0, record_trace=1)
        prm.loam_disable_cache = disable
        prm.loam_coresident = coresident
        out.append(_call(LoamRegister(params=prm), n_src, rung))
    return tuple(out)


def _assert_same(a, b, what):
    (pa, ca, ta), (pb, cb, tb) = a, b
    assert ca == cb, what
    assert ta["iters_run"] == tb["iters_run"], what
    for key in ("n", "JtJ", "JtE", "x"):
        assert np.array_equal(ta[key], tb[key]), (what, key)
    assert np.array_equal(pa, pb), what


def test_every_posting_shape_gives_the_uncached_result(gpu):
    seen = []
    for n_src in SINGLE_BLOCK:
        for rung in range(len(LADDER)):
            cached, plain = _pair(n_src, rung)
            srch = [int(v) for v in cached[2]["searches"]]
            print(f"n_src {n_src:3d} rung {rung}: searches per launch {srch}")
            _assert_same(cached, plain, (n_src, rung))
            assert all(0 <= v <= n_src for v in srch)
            seen += srch
    missing = [c for c in CLASSES if not any(c[0] <= v <= c[1] for v in seen)]
    assert not missing, f"miss counts never seen: {missing}"


@pytest.mark.parametrize("n_src", MULTI_BLOCK)
def test_two_and_three_blocks(gpu, n_src):
    for rung in (0, 3):
        cached, plain = _pair(n_src, rung)
        print(f"n_src {n_src} rung {rung}: searches per launch {[int(v) for v in cached[2]['searches']]}")
        _assert_same(cached, plain, (n_src, rung))
    # two consecutive identical calls on one handle: the fold order of the blocks' rows and the parity of the state
    reg = LoamRegister(loam_iters=ITERS, loam_early_exit=0, record_trace=1)
    first = _call(reg, n_src, 0)
    second = _call(reg, n_src, 0)
    _assert_same(first, second, (n_src, "repeat"))
    _assert_same(first, _pair(n_src, 0)[0], (n_src, "fresh handle"))


def test_coresident_instantiation(gpu):
    cached, plain = _pair(513, 0, coresident=1)
    _assert_same(cached, plain, "coresident")
    _assert_same(cached, _pair(513, 0)[0], "coresident against the default kernel")


def test_rows_against_the_oracle(gpu):
    """pcr_loam_linearize at 300 points (two blocks, the second partly filled), tolerances of tests/test_loam_gpu.py."""
    m, _, _ = _world()
    scan = _scan(300)
    reg = LoamRegister()
    reg.setTarget(m)
    tree = oracle.KdTree(m)
    for pose in (_init(1), _init(5)):
        g = reg.linearize(scan, pose, per_point=True)
        o = oracle.loam_linearize(tree, scan, pose, oracle.loam_params(), per_point=True)
        assert g["n"] == o["n"] > 6
        np.testing.assert_array_equal(g["status"], o["status"])
        acc = o["status"] == 0
        np.testing.assert_array_equal(g["nn"][acc], o["nn"][acc])
        np.testing.assert_allclose(g["rows"][acc], o["rows"][acc], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(g["JtJ"], o["JtJ"], rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(g["JtE"], o["JtE"], rtol=1e-9, atol=1e-9)


def test_few_writers_leave_whole_entries(gpu):
    """A launch in which a handful of lanes rewrite their entries stores them lane by lane.  An entry left stale or half written would be searched
    again by the next launch, or would change the pose."""
    n_src, rung = FEW_WRITER_CASE
    cached, plain = _pair(n_src, rung)
    srch = [int(v) for v in cached[2]["searches"]]
    print(f"searches per launch {srch}")
    few = [k for k in range(1, ITERS - 1) if 1 <= srch[k] <= 8]
    assert few, srch
    k = few[-1]
    assert srch[k + 1] == 0, srch
    assert np.array_equal(cached[0], plain[0])
