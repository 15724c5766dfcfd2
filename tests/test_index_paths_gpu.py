"""One index walked through its kinds of build (csrc/grid_index.hip: GridIndex::build, planned by csrc/grid_plan.h): fresh box -> tile size by the
cells seen -> header reused -> header and layout reused -> stale hint rebuilt; the same without hints; and the voxel filter's sparse, cut lattice.
A loam handle's kept target IS the index, so setTarget builds it and knn reads it: every answer is compared with brute force (tests/knn_ref.py, its
tie rule) exactly as tests/test_knn_query_gpu.py does -- indices equal, squared distances bit for bit.

The cloud, and the rule each part is there for (1 m cells):
  ~20 000 points over a 40 x 40 x 6 m box   the bulk: ~19 000 cells, so from the second build on tiles of 512 cells holding ~850 points on average --
                                             eight points per thread, tiles cut at hs = 2 048
  6 000 points over a 3 m cube              with the next part, the tile they share holds several times hs: the layout cuts that tile into slabs
  6 000 points inside a 0.2 m cube          one cell, which no cut divides: its slab stays heavier than the 4 096 points a block holds in registers
                                             and goes through the chunked path
"""
import numpy as np
import pytest

import knn_ref
import oracle
from simpleslam_amd import LoamRegister

pytestmark = pytest.mark.gpu

LO, HI = np.float32([-20, -20, -1]), np.float32([20, 20, 5])
CUBE = np.float32([3.3, -7.6, 0.4])       # lower corner of the 3 m cube; the 0.2 m cube sits inside it
TIGHT = CUBE + np.float32([1.3, 1.1, 0.9])


def _points(rng, n, lo, hi):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    p[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    return p


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(20261020)
    first = np.concatenate([_points(rng, 20000, LO, HI), _points(rng, 6000, CUBE, CUBE + 3), _points(rng, 6000, TIGHT, TIGHT + np.float32(0.2))])
    first[0, :3] = LO; first[1, :3] = HI      # the box is the same whatever the draw
    first = first[rng.permutation(len(first))]
    clouds = [first]
    for _ in range(3):      # a growing map: the last cloud + 500 points inside the box
        clouds.append(np.concatenate([clouds[-1], _points(rng, 500, LO + 1, HI - 1)]))
    stray = clouds[-1].copy()
    stray[777, :3] = HI + np.float32([30, 0, 0])      # 30 m outside the old box: the hinted header is stale
    clouds.append(stray)
    q = np.concatenate([first[np.flatnonzero((first[:, :3] >= CUBE).all(1) & (first[:, :3] <= CUBE + 3).all(1))[:200]],      # cluster points
                        _points(rng, 56, HI + 2, HI + 25), _points(rng, 56, LO - 25, LO - 2),                               # outside the box
                        np.round(_points(rng, 200, LO, HI))])                                                               # on cell faces (and edges, and corners)
    assert q.shape == (512, 4)
    want = [knn_ref.knn(c, q, 5) for c in clouds]
    return dict(clouds=clouds, queries=np.ascontiguousarray(q), want=want)


def _walk(case, **params):
    """setTarget + knn for the five clouds on one handle -> [(box hint, layout hint, idx, d2)]"""
    reg = LoamRegister(**params)
    out = []
    for cloud in case["clouds"]:
        reg.setTarget(cloud)
        st = reg.stats()
        idx, d2 = reg.knn(case["queries"], 5)
        out.append((st["index_box_hint"], st["index_layout_hint"], idx, d2))
    return out


@pytest.fixture(scope="module")
def hinted(gpu, case):
    return _walk(case)


def _exact(got, want):
    for j, ((_, _, idx, d2), (want_i, want_d)) in enumerate(zip(got, want)):
        print(f"cloud {j}: {int((idx != want_i).any(axis=1).sum())} of {len(idx)} rows differ from brute force")
        np.testing.assert_array_equal(idx, want_i, err_msg=f"cloud {j}")
        assert d2.dtype == want_d.dtype == np.float64 and d2.tobytes() == want_d.tobytes(), f"cloud {j}: distances differ in bits"


def test_growing_map_is_exact_on_every_kind_of_build(hinted, case):
    flags = [(b, l) for b, l, _, _ in hinted]
    print("box hint, layout hint per call:", flags)
    _exact(hinted, case["want"])
    assert flags[0] == (0, 0)                      # a fresh index has nothing to reuse
    assert flags[3] == (1, 1), flags               # by the fourth call the header and the layout are the previous build's: else this test has not walked the paths it is for
    assert all(l <= b for b, l in flags)


def test_stale_hint_is_rebuilt(hinted, case):
    assert hinted[3][0] == 1                       # the hint was in use ...
    assert (hinted[4][0], hinted[4][1]) == (0, 0)  # ... and the cloud with a point 30 m outside its box was indexed again, with a fresh box
    _exact(hinted[4:], case["want"][4:])


def test_without_hints_same_answers(gpu, hinted, case):
    plain = _walk(case, index_no_hints=1)
    assert [(b, l) for b, l, _, _ in plain] == [(0, 0)] * 5
    for j, (a, b) in enumerate(zip(plain, hinted)):
        np.testing.assert_array_equal(a[2], b[2], err_msg=f"cloud {j}")
        assert a[3].tobytes() == b[3].tobytes(), f"cloud {j}: distances differ in bits from the hinted run's"


def _voxel_ids(pts, leaf):
    """PCL voxel index of every row on the cloud's own lattice (float arithmetic as in voxel_grid.hpp)"""
    inv = np.float32(1.0) / np.float32(leaf)
    min_b = np.floor(pts[:, :3].min(0) * inv).astype(np.int64)
    div_b = np.floor(pts[:, :3].max(0) * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(pts[:, :3].astype(np.float32) * inv) - min_b.astype(np.float32)).astype(np.int64)
    return ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1], int(div_b.prod())


def test_voxel_filter_on_a_sparse_lattice(gpu, case):
    """Three clouds of ~20 000 points that differ by a few hundred, leaf 0.1 m: a lattice of 400 x 400 x 60 voxels, far more than 4 n + 65 536 cells, so from the
    second call on (the cell count is known then) the filter's index takes the sparse variants, cuts its heavy tiles and counts by runs.  Compared as
    tests/test_voxel_gpu.py compares."""
    rng = np.random.default_rng(7)
    base = case["clouds"][0][::2][:16000]
    corners = np.zeros((2, 4), np.float32)
    corners[0, :3] = LO; corners[1, :3] = HI
    base = np.concatenate([base, corners])      # (the same lattice for every cloud)
    reg = LoamRegister()
    leaf = 0.1
    for call in range(3):
        pts = np.concatenate([base, _points(rng, 3700 + 150 * call, LO + 1, HI - 1)])
        ids, cells = _voxel_ids(pts, leaf)
        assert cells > 4 * len(pts) + 65536
        got = reg.voxelDownSample(pts, leaf)
        ref, unfiltered = oracle.voxel_filter(pts, leaf)
        assert not unfiltered
        assert got.shape == ref.shape, call
        np.testing.assert_allclose(got[:, :3], ref[:, :3], rtol=0, atol=5e-4)
        np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=1e-3)
        order = np.argsort(ids, kind="stable")
        uniq, start, cnt = np.unique(ids[order], return_index=True, return_counts=True)
        assert len(uniq) == len(got)
        exact = (np.add.reduceat(pts[order, :3].astype(np.float64), start, axis=0) / cnt[:, None]).astype(np.float32)
        np.testing.assert_allclose(got[:, :3], exact, rtol=0, atol=1e-5)
