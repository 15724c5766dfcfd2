"""The inputs of tests/knn_cases.py held to the conditions they were made for, with tests/knn_ref.py alone (no GPU): these are what keeps
tests/test_knn_query_edges_gpu.py from passing vacuously.  The seeds are fixed in knn_cases so that every count below is met."""
import numpy as np
import pytest

import knn_cases
import knn_ref
import voxel_ref

# (cell, shift, float lattice) of the three handles as tests/test_knn_query_edges_gpu.py creates them
LATTICES = {"loam": (1.0, 0.0, False), "vgicp": (1.0, 0.5, False), "ndt": (float(np.float32(0.7)), 0.0, True)}


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_tie_queries_tie_at_every_k(which, copies):
    """Per lattice and k: at least 20 queries whose k-th and (k + 1)-th distances are equal (the cut goes through a block of equal
    distances), at least 20 with equal distances inside the list (k >= 2: a list of one has no inside), and at least 20 where a tied point
    that must be kept is stored after a tied point that must be dropped -- whoever keeps the first one met is wrong there."""
    lat = knn_cases.lattices(copies)[which]
    n = len(lat.target)
    assert n == 12 * 12 * 6 * copies
    assert (np.diff(lat.storage) < 0).sum() > n // 3      # the rows are not in the index's order
    for k in lat.values:
        kk = min(n, k + 80)      # the largest block of equal distances is 24 sites x 3 copies
        idx, d2 = knn_ref.knn(lat.target, lat.queries, kk)
        straddle = d2[:, k - 1] == d2[:, k]
        inside = (d2[:, :k - 1] == d2[:, 1:k]).any(axis=1)
        late = 0
        for j in np.flatnonzero(straddle):
            tied = np.flatnonzero(d2[j] == d2[j, k - 1])
            assert tied[-1] < kk - 1, "the block of equal distances does not end inside the k + 80 computed"
            kept, dropped = idx[j, tied[tied < k]], idx[j, tied[tied >= k]]
            assert kept.max() < dropped.min()      # the lower rows are the ones kept
            late += lat.storage[kept].max() > lat.storage[dropped].min()
        print(f"lattice {which} copies {copies} k {k}: {int(straddle.sum())} straddle, {int(inside.sum())} inside, {late} kept-but-stored-later, of {len(lat.queries)}")
        assert straddle.sum() >= 20
        assert k == 1 or inside.sum() >= 20
        assert late >= 20


def test_lattice_distances_are_the_ones_promised():
    lat = knn_cases.lattice(copies=1, seed=11)
    q = np.zeros((4, 4), np.float32)
    q[0, :3] = (5, 5, 3); q[1, :3] = (5.5, 5.5, 2.5); q[2, :3] = (5.5, 5.5, 3); q[3, :3] = (5.5, 5, 3)
    _, d2 = knn_ref.knn(lat.target, q, 33)
    np.testing.assert_array_equal(d2[0, :27], [0] + [1] * 6 + [2] * 12 + [3] * 8)
    np.testing.assert_array_equal(d2[1, :32], [0.75] * 8 + [2.75] * 24)
    np.testing.assert_array_equal(d2[2, :12], [0.5] * 4 + [1.5] * 8)
    np.testing.assert_array_equal(d2[3, :10], [0.25] * 2 + [1.25] * 8)


@pytest.mark.parametrize("centre", [knn_cases.NEAR, knn_cases.FAR])
@pytest.mark.parametrize("name", list(LATTICES))
def test_face_clouds_touch_the_faces(name, centre):
    cell, shift, float_lattice = LATTICES[name]
    fc = knn_cases.face_cloud(cell, shift, centre, seed=21, float_lattice=float_lattice)
    assert len(fc.target) <= 5000 and len(fc.queries) <= 3100
    for what, pts in (("target", fc.target), ("queries", fc.queries)):
        near = (knn_cases.ulps_from_a_face(pts[:, :3], cell, shift) <= 2).any(axis=1)
        each = [int((knn_cases.ulps_from_a_face(pts[:, :3], cell, shift)[:, ax] == u).sum()) for ax in range(3) for u in range(3)]
        print(f"{name} {centre} {what}: {int(near.sum())} of {len(pts)} within two ulps of a face; per axis and ulp distance {each}")
        assert near.sum() >= 50
        assert min(each) >= 5      # on the face, one and two ulps off it, on every axis
    if name == "ndt" and centre == knn_cases.FAR:
        d = voxel_ref.disagrees(fc.target[:, :3], np.float32(cell))
        print(f"ndt far: {int(d.any(axis=1).sum())} target points whose float cell differs from the f64 one")
        assert d.any(axis=1).sum() >= 1
        # the k-th neighbour is to lie across a face often: with 20 neighbours the list reaches into another cell
    _, d2 = knn_ref.knn(fc.target, fc.queries, 20)
    assert np.median(np.sqrt(d2[:, 19])) > 0.5 * cell


@pytest.mark.parametrize("centre", [knn_cases.NEAR, knn_cases.FAR])
def test_slop_probes_need_the_slop(centre):
    """The float lattice's probes, by a model of the search with a slop of zero: p lies below the slab of the cell float puts it into; the
    decoy is as far from the query as p and the slab farther, so a row skip on the bare slab distance loses p, which is the k = 1 answer
    (the lower row of the tie); q + radius falls short of the slab while p is inside the radius."""
    cell, shift, _ = LATTICES["ndt"]
    fc = knn_cases.face_cloud(cell, shift, centre, seed=21, float_lattice=True)
    T, Q = fc.target[:, :3].astype(np.float64), fc.queries[:, :3].astype(np.float64)
    idx, d2 = knn_ref.knn(fc.target, fc.queries, 2)
    knn_good, radius_good = {0: 0, 1: 0, 2: 0}, {0: 0, 1: 0, 2: 0}
    for g in fc.slop_probes:
        ax, r = g.ax, g.radius
        slab_lo = knn_cases.float_cell(fc.target[g.prows, ax], cell) * cell
        assert (slab_lo > T[g.prows, ax]).all() and (np.floor(T[g.prows, ax] / cell) * cell < T[g.prows, ax]).all()      # float's cell is not f64's
        np.testing.assert_array_equal(T[g.prows, ax] - Q[g.qrows, ax], g.d)
        np.testing.assert_array_equal(Q[g.qrows, ax] - T[g.drows, ax], g.d)
        np.testing.assert_array_equal(slab_lo - Q[g.qrows, ax], g.gap)
        assert 0 < g.d < r < g.gap and g.gap * g.gap >= r * r * (1.0 + 2.0 ** -40) and (g.prows < g.drows).all()
        knn_good[ax] += int(((idx[g.qrows, 0] == g.prows) & (idx[g.qrows, 1] == g.drows) & (d2[g.qrows, 0] == g.d * g.d) & (d2[g.qrows, 1] == g.d * g.d)).sum())
        off, ridx, _ = knn_ref.radius_search(fc.target, fc.queries[g.qrows], r, sorted_=False)
        radius_good[ax] += sum(int(g.prows[j] in ridx[int(off[j]):int(off[j + 1])]) for j in range(len(g.qrows)))
    print(f"{centre}: probes that need the slop, per axis: k = 1 {knn_good}, radius {radius_good}, in {len(fc.slop_probes)} groups")
    assert knn_good[1] >= 5 and knn_good[2] >= 5      # (the x axis skips no row in the k-NN search: its probes serve the radius search)
    assert min(radius_good.values()) >= 5


def test_shells_give_every_segment_length():
    sh = knn_cases.shells(2500, seed=31)
    assert len(sh.target) <= 5000
    assert (np.diff(sh.dist[:2501]) > 5e-4).all()      # strictly increasing, well separated: float32 moves a point by 1e-6 at most
    cell = np.floor(sh.target[:, :3].astype(np.float64))
    c = np.floor(np.asarray(sh.centre))
    assert ((cell[:, 1:] == c[1:]).all(axis=1)).sum() >= 2500 and (cell == c).all(axis=1).sum() > 4 * 64      # one row, one cell
    for m in knn_cases.SHELL_LENGTHS:
        off, idx, d2 = knn_ref.radius_search(sh.target, sh.queries, sh.radius(m))
        np.testing.assert_array_equal(off, [0, m, m, 2 * m])


def test_mixed_queries_straddle_the_scan_seams():
    target = knn_cases.random_cloud(4000, seed=41)
    for n in knn_cases.MIXED_SIZES:
        mq = knn_cases.mixed_queries(n, target, seed=42)
        assert len(mq.queries) == n
        off, _, _ = knn_ref.radius_search(target, mq.queries, mq.values)
        cnt = np.diff(off.astype(np.int64))
        assert (cnt[mq.kind == knn_cases.OUT] == 0).all() and (cnt[mq.kind == knn_cases.BAD] == 0).all()
        assert (cnt[mq.kind == knn_cases.COPY] >= 1).all()
        for s in (1024, 2048):
            if n >= s + 4:
                for side in (cnt[s - 4:s], cnt[s:s + 4]):
                    assert (side == 0).any() and (side > 0).any()
        if n >= 1024:
            assert cnt[:1024].sum() > 0      # a carry to hand on
        if n >= 100:
            for kd in (knn_cases.IN, knn_cases.OUT, knn_cases.BAD, knn_cases.COPY):
                assert (mq.kind == kd).sum() >= n // 10
            assert (cnt > 0).sum() >= n // 3 and (cnt == 0).sum() >= n // 3
