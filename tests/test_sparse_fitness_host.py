"""The fitness scores' search on the sparse target index (csrc/sparse_fitness.hip), on the CPU: the `fitness` mode of host/sparse_index_check.cpp runs
the walk of csrc/sparse_walk.h with K = 1 under the visitor the kernels compile (sw::NearestF32: the least FLOAT squared distance within the gate)
and a brute force over every stored point beside it.  Here each answer is also compared, bit for bit, with numpy's brute force (fitness_ref.py: the
reference of every score test), on the two-cluster cloud, the stray-point cloud and a compact one, with the gate of 1 m^2 and without one; the walk's
look-ups are held to its stated bound (102 for the rings, 1 for the seed, 1 + 5 R + 2 L for a box scan over R occupied rows in L occupied layers), and
with the gate a query kilometres from every point must cost the rings' look-ups and nothing more.

The adversarial queries go at the one thing new in this search: its bounds are exact f64 distances, its answer a float distance that may lie below
the exact one (by less than 5 x 2^-24 of it: sparse_walk.h at the visitor).  Queries on cell faces (a bound of exactly 0 or exactly one cell), and
pairs of points in DIFFERENT rows at exactly the same f64 distance from their query whose float distances differ by an ulp, either way round --
(a, b, c) and (c, -a, b) off the query, with a, b, c chosen so that fl(fl(a a + b b) + c c) != fl(fl(c c + a a) + b b) -- near the origin and at
+-30 km, where a float step is 2 mm: a walk that ended on the first of such a pair, or ranked them in f64, would return the larger."""
import os
import re
import subprocess

import numpy as np
import pytest

import fitness_ref as fr
import sparse_index_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "sparse_index_check")
NONE = np.float32(3.0e38)
FLT_MAX = float(np.finfo(np.float32).max)
GATES = (1.0, FLT_MAX)


def _f32_sum(a, b, c):
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    return np.float32(np.float32(a * a + b * b) + c * c)


def ulp_pairs(centre, step, kmax, count, seed):
    """`count` (query, p1, p2): p1 = q + (a, b, c), p2 = q + (c, -a, b), a, b, c multiples of `step` (so that q + a is a float and q - p exact), at one
    f64 distance from q and with float distances one rounding apart; half with p1 the nearer in float, half with p2"""
    rng = np.random.default_rng(seed)
    q = np.asarray(centre, np.float64)
    out, want_first = [], True
    while len(out) < count:
        a, b, c = (rng.integers(1, kmax, 3) * step).astype(np.float64)
        d1, d2 = _f32_sum(a, b, c), _f32_sum(c, a, b)
        if d1 == d2 or (d1 < d2) != want_first:
            continue
        p1, p2 = q + (a, b, c), q + (c, -a, b)
        for p in (p1, p2):      # the construction's premises, checked: the points are floats, and the float differences are the exact ones
            assert (p.astype(np.float32).astype(np.float64) == p).all()
        assert a * a + b * b + c * c == c * c + a * a + b * b and np.floor(p1[1]) != np.floor(p2[1])
        out.append((q.copy(), p1, p2))
        want_first = not want_first
        q = q + (0.0, 0.0, 40.0)      # the next pair well away from this one
    return out


def adversarial(seed=0):
    """points and queries of the ulp pairs: at the origin (steps of 2^-12 up to 1 m), at +30 km and at -30 km (steps of 2^-9 = 2 mm up to 8 m)"""
    pts, qs = [], []
    for centre, step, kmax in (((10.0, 10.0, 10.0), 2.0 ** -12, 4096), ((30010.0, 20010.0, 8010.0), 2.0 ** -9, 4096),
                               ((-30010.0, -20010.0, -8010.0), 2.0 ** -9, 4096)):
        for q, p1, p2 in ulp_pairs(centre, step, kmax, 12, seed):
            qs.append(q); pts += [p1, p2]
        seed += 1
    return cases.cloud(np.array(pts)), cases.cloud(np.array(qs))


def face_queries(target, seed, n=16):
    """queries on cell faces and lattice points beside stored points: integer coordinates, one axis, two or all three"""
    t = target[np.isfinite(target[:, :3]).all(axis=1), :3].astype(np.float64)
    rng = np.random.default_rng(seed)
    q = t[rng.integers(0, len(t), n)].copy()
    for i in range(n):
        axes = [(0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)][i % 6]
        for a in axes:
            q[i, a] = np.floor(q[i, a]) + (i % 2)
    return cases.cloud(q)


def run_fitness(tmp_path, target, queries, gate):
    assert os.path.exists(EXE), "build() makes it (csrc/Makefile: harness)"
    np.ascontiguousarray(target, np.float32).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(queries, np.float32).tofile(tmp_path / "q.f32")
    out = subprocess.run([EXE, "fitness", str(tmp_path / "t.f32"), str(tmp_path / "q.f32"), repr(float(gate))], capture_output=True, text=True, timeout=300)
    rows = []
    for line in out.stdout.splitlines():
        if line.startswith("q "):
            w = line.split()
            rows.append({w[i]: int(w[i + 1]) for i in range(2, len(w), 2)})
    return out, rows


def check(tmp_path, target, queries):
    """every answer the brute force's (the program's own and numpy's), every walk within its bound; returns the rows of the gated run"""
    want, _ = fr.nearest_sq(queries[:, :3], target)
    finite = np.isfinite(queries[:, :3]).all(axis=1)
    gated = None
    for gate in GATES:
        out, rows = run_fitness(tmp_path, target, queries, gate)
        assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-600:] + out.stderr
        assert len(rows) == len(queries)
        assert tuple(map(int, re.search(r"bounds ring (\d+) row (\d+) layer (\d+)", out.stdout).groups())) == (102, 5, 2)
        got = np.array([r["got"] for r in rows], np.uint32).view(np.float32)
        with np.errstate(invalid="ignore"):
            ref = np.where(finite & (want <= np.float32(gate)) & (want < NONE), want, NONE).astype(np.float32)
        assert got.tobytes() == ref.tobytes(), (gate, np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0][:8])
        for j, r in enumerate(rows):
            cap = 102 + 1 + r["box"] * (1 + 5 * r["rows"] + 2 * r["layers"])
            assert r["lookups"] <= cap, (gate, j, r, cap)
            if not finite[j]:
                assert r["lookups"] == 0
        if gate == 1.0:
            gated = rows
    return gated


def test_two_clusters_30_km_apart(tmp_path):
    t = cases.two_clusters()
    q = np.vstack([cases.queries_for(t, seed=1), face_queries(t, 2)])
    gated = check(tmp_path, t, q)
    # with the gate, no query comes to the seed or the box scan: halfway between the clusters and 15 km outside the box it is the rings and nothing more
    assert all(r["box"] == 0 and r["lookups"] <= 102 for r in gated), max(r["lookups"] for r in gated)
    far = [r for r, row in zip(gated, q) if np.isfinite(row[:3]).all() and fr.nearest_sq(row[None, :3], t)[0][0] > 1e6]
    assert len(far) >= 3 and all(r["got"] == int(NONE.view(np.uint32)) and r["points"] == 0 for r in far)


def test_stray_point_at_4e6_m(tmp_path):
    """(beside the stray point the faces' slop is metres wide: there a gated walk may come to the box scan, within its bound)"""
    t = cases.stray()
    q = np.vstack([cases.queries_for(t, seed=5), face_queries(t, 6), t[len(t) // 2][None] + np.float32([0.5, 0.25, -0.5, 0.0])])
    gated = check(tmp_path, t, q)
    near = np.abs(q[:, :3]).max(axis=1) < 1e5
    assert all(r["box"] == 0 and r["lookups"] <= 102 for r, ok in zip(gated, near) if ok)


@pytest.mark.parametrize("n", [1, 2, 2049])
def test_compact_cloud_with_faces_duplicates_and_ties(tmp_path, n):
    t = cases.edge_cloud(n, seed=n)
    if n > 2:
        t[n // 2, 1] = np.nan
    q = np.vstack([cases.queries_for(t, seed=n + 1), face_queries(t, n + 2)])
    gated = check(tmp_path, t, q)
    assert all(r["box"] == 0 and r["lookups"] <= 102 for r in gated)


def test_equal_in_f64_one_ulp_apart_in_float(tmp_path):
    pts, qs = adversarial()
    t = np.vstack([cases.edge_cloud(500, seed=9), pts])      # (30 km apart: a box no dense table holds, and a compact cloud around the first pairs)
    d, idx = fr.nearest_sq(qs[:, :3], t)
    pair = (idx - 500) // 2
    assert (idx >= 500).all() and (pair == np.arange(len(qs))).all()      # the nearest point of each query is one of its own pair
    first = ((idx - 500) % 2 == 0)
    assert 12 <= first.sum() <= 24 and 12 <= (~first).sum() <= 24         # ... the first of the pair for half of them, the second for the others
    other = t[500 + 2 * pair + first.astype(int), :3]
    d_other = fr.sq_dist_f32(qs[:, :3], other)[np.arange(len(qs)), np.arange(len(qs))]
    assert (d_other > d).all() and (d_other == np.nextafter(d, np.float32(np.inf))).sum() >= 12      # an ulp apart (a rounding: one or two)
    check(tmp_path, t, qs)
    check(tmp_path, t[::-1].copy(), qs)      # the other order of rows
