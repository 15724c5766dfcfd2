"""k-nearest-neighbour and radius search by brute force, in numpy float64: the plain reference pcr_knn and pcr_radius_search are checked
against (tests/test_knn_query_gpu.py), itself pinned to the reference's nanoflann (tests/test_knn_ref.py).

nanoflann::PointCloudKdtree<PointXYZI, double> (pcl_adaptor.hpp:11-78) hands nanoflann float coordinates as doubles
(kdtree_get_pt returns Scalar = double) and metric_L2_Simple accumulates (a - b)^2 over x, y, z in double.  Here every step rounds
the same way:

- target and query coordinates are float32 values widened to float64;
- d2 = (dx dx + dy dy) + dz dz in float64, each product and sum rounded on its own (numpy does not fuse);
- target points with a coordinate that is not finite are left out; the others keep their row number;
- results ascend by (d2, row): among equal distances the lower row first (nanoflann's own tie order follows its tree walk);
- knn: fewer than k points, or a query with a coordinate that is not finite: row -1, distance +inf;
- radius: d2 < radius * radius, strict (RadiusResultSet::addPoint), the square taken in float64 (pcl_adaptor.hpp:65).
"""
import numpy as np


def _xyz64(cloud):
    a = np.asarray(cloud, np.float32)
    return a.reshape(a.shape[0], -1)[:, :3].astype(np.float64)


def _d2_rows(q, pts):
    """(len(q), len(pts)) float64 squared distances, accumulated in the reference's order"""
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - pts[None, :, 0]
        d = dx * dx
        dy = q[:, None, 1] - pts[None, :, 1]
        d += dy * dy
        dz = q[:, None, 2] - pts[None, :, 2]
        d += dz * dz
    return d


def knn(pts, queries, k, chunk=256):
    """-> (idx (n, k) int64, d2 (n, k) float64)"""
    P, Q = _xyz64(pts), _xyz64(queries)
    rows = np.flatnonzero(np.isfinite(P).all(axis=1))
    P = P[rows]
    idx = np.full((Q.shape[0], k), -1, np.int64)
    d2 = np.full((Q.shape[0], k), np.inf, np.float64)
    ok = np.isfinite(Q).all(axis=1)
    m = min(k, len(rows))
    if m == 0:
        return idx, d2
    for s in range(0, Q.shape[0], chunk):
        sel = np.flatnonzero(ok[s:s + chunk]) + s
        if len(sel) == 0:
            continue
        d = _d2_rows(Q[sel], P)
        # rows ascend, so a stable sort by distance orders equal distances by row
        order = np.argsort(d, axis=1, kind="stable")[:, :m]
        idx[sel, :m] = rows[order]
        d2[sel, :m] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def radius_search(pts, queries, radius, sorted_=True, chunk=256):
    """-> (offsets (n + 1,) uint64, idx int64, d2 float64); unsorted segments ascend by row"""
    P, Q = _xyz64(pts), _xyz64(queries)
    rows = np.flatnonzero(np.isfinite(P).all(axis=1))
    P = P[rows]
    r2 = np.float64(radius) * np.float64(radius)
    ok = np.isfinite(Q).all(axis=1)
    li, ld, counts = [], [], np.zeros(Q.shape[0], np.uint64)
    for s in range(0, Q.shape[0], chunk):
        d = _d2_rows(Q[s:s + chunk], P)
        for j in range(d.shape[0]):
            if not ok[s + j]:
                continue
            hit = np.flatnonzero(d[j] < r2)
            dd = d[j, hit]
            if sorted_:
                o = np.argsort(dd, kind="stable")
                hit, dd = hit[o], dd[o]
            li.append(rows[hit]); ld.append(dd); counts[s + j] = len(hit)
    offsets = np.zeros(Q.shape[0] + 1, np.uint64)
    offsets[1:] = np.cumsum(counts)
    idx = np.concatenate(li).astype(np.int64) if li else np.zeros(0, np.int64)
    d2 = np.concatenate(ld) if ld else np.zeros(0, np.float64)
    return offsets, idx, d2
