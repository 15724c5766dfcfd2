"""The fitness score by brute force, in numpy float32: the plain reference the device's 1-NN search is checked against.

pcl::Registration::getFitnessScore (VgicpRegister.cpp:42-45) and the gated score of the reference's test/align.cpp:29-61 are both
the mean squared distance from each transformed source point to its nearest target point, over the points whose distance passes
the gate.  Here every step rounds as the reference does:

- the source is transformed with the pose cast to float32, ((T0 x + T4 y) + T8 z) + T12 per row (pcl::transformPointCloud in float);
- a squared distance is (dx dx + dy dy) + dz dz in float32, dx = q - p (FLANN's L2_Simple<float>);
- the minimum is taken over the FINITE target points (the kd-tree and the grid leave the others out), in chunks;
- a point counts when (double) d2 <= max_sq (a float distance against a double gate, as in PCL);
- the sum is taken in float64.  No point counted: -1 for the gated score, DBL_MAX for getFitnessScore.

numpy's float32 arithmetic rounds every product and sum on its own (no FMA), so each per-point distance is the reference's bit for bit.
"""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def _xyz(cloud):
    a = np.asarray(cloud, np.float32)
    return a.reshape(a.shape[0], a.shape[1] if a.ndim == 2 else 3)[:, :3]


def transform_f32(src, pose):
    """(n, 3) float32: the source's first three columns transformed by `pose` (4x4, map <- source) in float."""
    p = _xyz(src)
    Tf = np.asarray(pose, np.float64).astype(np.float32)
    q = np.empty((p.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            q[:, r] = ((Tf[r, 0] * p[:, 0] + Tf[r, 1] * p[:, 1]) + Tf[r, 2] * p[:, 2]) + Tf[r, 3]
    return q


def sq_dist_f32(q, t):
    """(len(q), len(t)) float32 squared distances, (dx dx + dy dy) + dz dz with dx = q - p: the one float expression of this project's
    brute-force references (FLANN's L2_Simple<float>)."""
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - t[None, :, 0]
        dy = q[:, None, 1] - t[None, :, 1]
        dz = q[:, None, 2] - t[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def nearest_sq(q, dst, chunk_elems=1 << 22):
    """Float32 squared distance from each query (n, 3 float32) to its nearest finite target point, and that point's row in `dst`
    (the lowest row among exact ties).  No finite target point: (inf, -1).  A query with a coordinate that is not finite: a NaN or
    inf distance, which no gate passes."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    t = _xyz(dst)
    rows = np.nonzero(np.isfinite(t).all(axis=1))[0]
    t = t[rows]
    d2 = np.full(q.shape[0], np.inf, np.float32)
    idx = np.full(q.shape[0], -1, np.int64)
    if t.shape[0] == 0 or q.shape[0] == 0:
        return d2, idx
    step = max(1, chunk_elems // t.shape[0])
    with np.errstate(all="ignore"):
        for a in range(0, q.shape[0], step):
            d = sq_dist_f32(q[a:a + step], t)
            j = np.argmin(np.where(np.isnan(d), np.float32(np.inf), d), axis=1)      # (first minimum: the lowest row)
            d2[a:a + step] = d[np.arange(d.shape[0]), j]
            idx[a:a + step] = rows[j]
    return d2, idx


def gated_from_sq(d2, max_sq):
    """(score, n_in) of the gated fitness from per-point float squared distances: mean of those with (double) d2 <= max_sq, -1 when none."""
    d = np.asarray(d2, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = d <= float(max_sq)
    n = int(keep.sum())
    return (float(d[keep].sum()) / n if n else -1.0), n


def fitness_gated(src, dst, pose, max_sq=DBL_MAX):
    """pcr_fitness_gated / the score of test/align.cpp: (score, n_in), score -1 when no point passes the gate."""
    d2, _ = nearest_sq(transform_f32(src, pose), dst)
    return gated_from_sq(d2, max_sq)


def fitness_score(src, dst, pose):
    """pcl::Registration::getFitnessScore (pcr_fitness): DBL_MAX when no point has a neighbour."""
    s, n = fitness_gated(src, dst, pose)
    return s if n else DBL_MAX


def sum_order_rtol(n):
    """Relative difference two means of the same n non-negative float64 terms, summed in different orders, can show: each sum is within
    (n - 1) 2^-53 of the exact one, and the division adds an ulp."""
    return (max(int(n), 1) + 2) * 2.0 ** -52
