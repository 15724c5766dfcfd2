"""The walk of the sparse target index (csrc/sparse_walk.h) on the CPU: host/sparse_index_check.cpp builds the index with a plain sort, answers
every query by the walk the kernels of csrc/sparse_index.hip compile too, and this file compares each answer with brute force (knn_ref.py)
-- indices equal, squared distances bit for bit -- and holds the walk's look-ups to the bound of its design: for the box scan
1 + 5 R + 2 L look-ups, R the occupied rows of the (z, y) range of the block scanned and L the occupied layers of its z range (sparse_walk.h,
at box_scan, says where 5 and 2 come from), plus at most 102 for the two rings and one for the seed of a k-NN walk.  A walk whose cost grew
with the EMPTY space between the query and the points -- a ring search stepping cell by cell over 15 km -- would exceed it a thousandfold;
on a GPU that would be a hang."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref
import sparse_index_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "sparse_index_check")


def _run(tmp_path, target, queries, k, radius):
    assert os.path.exists(EXE), "build() makes it (csrc/Makefile: harness)"
    np.ascontiguousarray(target, np.float32).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(queries, np.float32).tofile(tmp_path / "q.f32")
    out = subprocess.run([EXE, str(tmp_path / "t.f32"), str(tmp_path / "q.f32"), str(k), repr(float(radius)), str(tmp_path / "o.bin")],
                         capture_output=True, text=True, timeout=300)
    return out


def _answers(tmp_path, nq, k):
    raw = np.fromfile(tmp_path / "o.bin", np.uint8)
    at = 0

    def take(count, dtype):
        nonlocal at
        a = raw[at:at + 8 * count].view(dtype)
        at += 8 * count
        return a
    kidx = take(nq * k, np.int64).reshape(nq, k)
    kd2 = take(nq * k, np.float64).reshape(nq, k)
    off = take(nq + 1, np.uint64)
    total = int(off[-1])
    ridx, rd2 = take(total, np.int64), take(total, np.float64)
    assert at == len(raw)
    return kidx, kd2, off, ridx, rd2


def _counts(stdout):
    rows = []
    for line in stdout.splitlines():
        if line.startswith("q "):
            w = line.split()
            rows.append({w[i]: int(w[i + 1]) for i in range(2, len(w), 2)})
    ring, row, layer = map(int, re.search(r"bounds ring (\d+) row (\d+) layer (\d+)", stdout).groups())
    return rows, ring, row, layer


def _check(tmp_path, target, queries, k, radius):
    out = _run(tmp_path, target, queries, k, radius)
    assert out.returncode == 0, out.stdout[-400:] + out.stderr
    nq = len(queries)
    kidx, kd2, off, ridx, rd2 = _answers(tmp_path, nq, k)
    want_i, want_d = knn_ref.knn(target, queries, k)
    np.testing.assert_array_equal(kidx, want_i)
    assert kd2.tobytes() == want_d.tobytes()
    w_off, w_idx, w_d2 = knn_ref.radius_search(target, queries, radius, sorted_=True)
    np.testing.assert_array_equal(off, w_off)
    np.testing.assert_array_equal(ridx, w_idx)
    assert rd2.tobytes() == w_d2.tobytes()
    rows, ring, row, layer = _counts(out.stdout)
    assert len(rows) == nq and (ring, row, layer) == (102, 5, 2)
    worst = 0
    for j, c in enumerate(rows):
        knn_cap = ring + 1 + c["knn_box"] * (1 + row * c["knn_rows"] + layer * c["knn_layers"])
        rad_cap = c["rad_box"] * (1 + row * c["rad_rows"] + layer * c["rad_layers"])
        assert c["knn_lookups"] <= knn_cap, (j, c, knn_cap)
        assert c["rad_lookups"] <= rad_cap, (j, c, rad_cap)
        worst = max(worst, c["knn_lookups"])
    finite = np.isfinite(queries[:, :3]).all(axis=1)
    assert all(c["knn_lookups"] == 0 and c["rad_lookups"] == 0 for c, f in zip(rows, finite) if not f)
    return rows, worst


@pytest.mark.parametrize("k", [1, 8, 9, 32])
def test_two_clusters_30_km_apart(tmp_path, k):
    """every answer exact, and the far queries -- halfway between the clusters, 15 km outside the box -- within the look-up bound: the clusters
    hold a few hundred occupied rows, the space between them 4.8e12 empty cells"""
    t = cases.two_clusters()
    q = cases.queries_for(t, seed=k)
    rows, worst = _check(tmp_path, t, q, k, 40000.0)
    far = [c for c in rows if c["knn_box"]]
    assert far, "no query reached the box scan: the far queries are not far"
    print(f"k = {k}: worst k-NN walk {worst} look-ups; far queries: " + ", ".join(f"{c['knn_lookups']} ({c['knn_rows']} rows)" for c in far))
    assert worst < 20000      # (600 points cannot occupy more than 600 rows: 102 + 2 + 5 x 600 + 2 x 600 at the very most)


@pytest.mark.parametrize("radius", [0.5, 3.0])
def test_stray_point_at_4e6_m(tmp_path, radius):
    t = cases.stray()
    _check(tmp_path, t, cases.queries_for(t, seed=5), 8, radius)


@pytest.mark.parametrize("n", [1, 2, 63, 65, 2049])
def test_faces_duplicates_ties_and_fewer_points_than_k(tmp_path, n):
    t = cases.edge_cloud(n, seed=n)
    t[n // 2, 1] = np.nan if n > 2 else t[n // 2, 1]      # a target row that is not finite renumbers nothing
    q = cases.queries_for(t, seed=n + 1)
    _check(tmp_path, t, q, 9, 3.0)
    _check(tmp_path, t, q[:8], 32, 0.5)


def test_a_stray_point_at_3e38_m_is_refused_with_the_extents(tmp_path):
    t = cases.stray(at=3.0e38)
    out = _run(tmp_path, t, t[:4], 1, 1.0)
    assert out.returncode == 3, out.stdout + out.stderr
    assert re.search(r"refused range 3e\+38 x \S+ x 3e\+38", out.stdout), out.stdout
    t = cases.stray(at=3.0e9)      # 32 + 5 + 32 key bits
    out = _run(tmp_path, t, t[:4], 1, 1.0)
    assert out.returncode == 3 and "refused bits" in out.stdout, out.stdout + out.stderr


def test_the_abi_declares_the_new_entry_point_and_parameter():
    from simpleslam_amd import pcr
    L = pcr.load_library()
    assert "pcr_query_index_info" in pcr.ABI_SYMBOLS and hasattr(L, "pcr_query_index_info")
    p = pcr.default_params()
    assert p.struct_size == C.sizeof(pcr.PcrParams) and p.query_index == pcr.QUERY_INDEX_AUTO == 0 and pcr.QUERY_INDEX_SPARSE == 1
    p.query_index = 2
    assert not L.pcr_create(b"loam", C.byref(p))
    assert b"query_index" in L.pcr_last_error(None)
