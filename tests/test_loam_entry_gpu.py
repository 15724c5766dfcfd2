"""The LOAM neighbour cache as it lies in memory -- tiles of 64 entries, ordered [field][lane] -- and the single barrier between the pose
update and the hit test, at the shapes where either can go wrong.

What is compared is exact: the cache decides WHO searches a query, never what a search returns, so a call with the cache must give the pose,
the per-launch sums and the steps of the same call on a handle without it (loam_disable_cache = 1), bit for bit.  A field read from the wrong
tile, a stale tile, or a staging area overwritten before it was read would change a hit into a wrong neighbourhood and with it the sums."""
import functools

import numpy as np
import pytest

from simpleslam_amd import LoamRegister, pcr, synth

pytestmark = pytest.mark.gpu

SEED = 7
ITERS = 6
# initial perturbation (metres, degrees): a first guess (its step is a big one: launch 1 searches everything again), a small one, and
# one whose later launches refit a handful of planes
LADDER = ((0.3, 2.0), (0.01, 0.1), (0.03, 0.3))
BIG, SMALL, FEW = 0, 1, 2
TILE_EDGES = (1, 63, 64, 65, 255, 256, 257, 320)
GRID_STRIDE = 512 * 256 + 65      # more scan points than 512 blocks of 256 take in one round


@functools.lru_cache(maxsize=None)
def _world():
    world, m = synth.make_map(20_000, seed=SEED)
    scan, T = synth.make_scan(world, 0, seed=SEED, beams=16, azimuths=128)
    big, _ = synth.make_scan(world, 0, seed=SEED, beams=64, azimuths=1024)      # same pose, 65 536 points
    for v in (m, scan, big, T):
        v.setflags(write=False)
    return m, scan, big, T


@functools.lru_cache(maxsize=None)
def _scan(n_src):
    _, scan, big, _ = _world()
    if n_src <= len(scan):
        s = np.ascontiguousarray(scan[np.linspace(0, len(scan) - 1, n_src).astype(int)])      # spread over the whole sweep
    else:
        s = np.ascontiguousarray(np.concatenate([big] * (n_src // len(big) + 1))[:n_src])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _init(rung):
    T = _world()[3]
    trans, rot = LADDER[rung]
    T0 = synth.perturb(T, SEED + rung, trans=trans, rot_deg=rot)
    T0.setflags(write=False)
    return T0


def _columns(a, cols):
    """The cloud with a point stride of 4 * cols bytes."""
    a = np.asarray(a)
    if cols <= a.shape[1]:
        return np.ascontiguousarray(a[:, :cols])
    return np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), cols - a.shape[1]), a.dtype)], axis=1))


def _reg(disable=0, coresident=0):
    prm = pcr.default_params(loam_iters=ITERS, loam_early_exit=0, record_trace=1)
    prm.loam_disable_cache = disable
    prm.loam_coresident = coresident
    return LoamRegister(params=prm)


def _call(reg, n_src, rung, cols=None):
    m, scan = _world()[0], _scan(n_src)
    if cols is not None:
        m, scan = _columns(m, cols), _columns(scan, cols)
    pose = _init(rung).copy()
    conv = reg.scan2Map(scan, m, pose)
    return pose, conv, reg.trace()


@functools.lru_cache(maxsize=None)
def _pair(n_src, rung, coresident=0, cols=None):
    """(cached, uncached) results of one call: computed once, shared by the tests below."""
    return tuple(_call(_reg(disable, coresident), n_src, rung, cols) for disable in (0, 1))


def _assert_same(a, b, what):
    (pa, ca, ta), (pb, cb, tb) = a, b
    assert ca == cb, what
    assert ta["iters_run"] == tb["iters_run"], what
    for key in ("n", "JtJ", "JtE", "x"):
        assert np.array_equal(ta[key], tb[key]), (what, key)
    assert np.array_equal(pa, pb), what


def _searches(res):
    return [int(v) for v in res[2]["searches"]]


@pytest.mark.parametrize("n_src", TILE_EDGES)
def test_tile_edges(gpu, n_src):
    """Partial last tiles, a block whose last wave is empty, a block with one valid lane."""
    for rung in (BIG, SMALL, FEW):
        cached, plain = _pair(n_src, rung)
        srch = _searches(cached)
        print(f"n_src {n_src} rung {rung}: searches per launch {srch} hits {[int(v) for v in cached[2]['cache_hits']]}")
        _assert_same(cached, plain, (n_src, rung))
        assert all(0 <= v <= n_src for v in srch)
        assert not np.any(plain[2]["cache_hits"]), "the uncached call hit"


def test_grid_stride_rounds(gpu):
    """More than kMaxPartials blocks' worth of scan points: the later rounds of a launch gather and store their tiles through the accessor."""
    for rung in (BIG, SMALL):
        cached, plain = _pair(GRID_STRIDE, rung)
        print(f"rung {rung}: searches per launch {_searches(cached)}")
        _assert_same(cached, plain, ("grid stride", rung))
        assert int(np.sum(cached[2]["cache_hits"])) > 512 * 256, "the later rounds never hit"


@pytest.mark.parametrize("cols", (3, 4))
def test_scan_stride(gpu, cols):
    """Scan points 12 and 16 bytes apart."""
    for n_src in (65, 320):
        cached, plain = _pair(n_src, SMALL, 0, cols)
        _assert_same(cached, plain, (cols, n_src))
    _assert_same(_pair(320, SMALL, 0, 3)[0], _pair(320, SMALL, 0, 4)[0], "the stride does not change the result")


def test_both_instantiations(gpu):
    for rung in (BIG, FEW):
        cached, plain = _pair(257, rung, coresident=1)
        _assert_same(cached, plain, ("coresident", rung))
        _assert_same(cached, _pair(257, rung)[0], ("coresident against the default kernel", rung))


@pytest.mark.parametrize("n_src", (256, 320))
def test_big_step_then_hits(gpu, n_src):
    """A first step large enough that launch 1 gives up the cache (kBigStep): its staging area is fetched and never used, and the launches
    behind it hit again."""
    cached, plain = _pair(n_src, BIG)
    srch, hits = _searches(cached), [int(v) for v in cached[2]["cache_hits"]]
    print(f"searches {srch} hits {hits}")
    _assert_same(cached, plain, n_src)
    assert hits[1] == 0 and srch[1] == srch[0] == n_src, "launch 1 did not take the big-step route"
    assert all(h > 0 for h in hits[2:]) and len(hits) > 2, "the launches behind the big step do not hit"


def test_few_writers_and_many_writers(gpu):
    """A launch in which a handful of lanes rewrite their entries and one in which all do, both through the same masked stores."""
    seen_few = seen_all = False
    for n_src, rung in ((256, FEW), (320, FEW), (257, BIG)):
        cached, plain = _pair(n_src, rung)
        srch = _searches(cached)
        print(f"n_src {n_src} rung {rung}: searches per launch {srch}")
        _assert_same(cached, plain, (n_src, rung))
        waves = (n_src + 63) // 64
        few = [k for k in range(1, ITERS - 1) if 1 <= srch[k] <= 8 * waves]
        seen_few |= bool(few)
        seen_all |= srch[0] == n_src
    assert seen_few and seen_all
    # what the few wrote is whole: the launch behind the last of them finds every entry in place (the case tests/test_loam_body_gpu.py pins too)
    srch = _searches(_pair(256, FEW)[0])
    few = [k for k in range(1, ITERS - 1) if 1 <= srch[k] <= 8]
    assert few and srch[few[-1] + 1] == 0, srch


def test_stale_tiles_across_calls(gpu):
    """Two scans of different length, the longer first, through one handle: the second equals a fresh handle's result."""
    reg = _reg()
    _call(reg, 320, BIG)
    second = _call(reg, 65, SMALL)
    _assert_same(second, _pair(65, SMALL)[0], "after a longer scan")
    _assert_same(second, _pair(65, SMALL)[1], "after a longer scan, against the uncached call")


def test_handle_reuse_at_growth(gpu):
    """64 points, then 65 536 on the same handle: the cache buffer grows by whole tiles."""
    reg = _reg()
    first = _call(reg, 64, SMALL)
    _assert_same(first, _pair(64, SMALL)[0], "64 points")
    grown = _call(reg, 65536, BIG)
    fresh, plain = _pair(65536, BIG)
    print(f"searches per launch {_searches(grown)}")
    _assert_same(grown, fresh, "grown handle against a fresh one")
    _assert_same(grown, plain, "grown handle against the uncached call")
