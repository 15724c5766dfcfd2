"""Reference ranking of stored ScanContexts against each other, over oracle.ScanContextOracle (the CPU restatement of
backend/src/ScanContext.cpp): what pcr_sc_rank_stored and the mirrors' findLoops must return.

rank(orc, first, count, k): for every query q of [first, first + count) and every candidate i of [0, q - num_exclude_recent),
orc.distance(q, i) -- the query unshifted, the candidate shifted -- and of those the k best by (dist, i) ascending; rows with fewer
than k candidates end in idx -1, dist DBL_MAX, shift 0.  find_loops applies query's threshold (strict) and forms its yaw."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def make_scan(seed, n=400, reach=90.0):
    """a few hundred points, as _scan of tests/test_scancontext_gpu.py builds them"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 8), np.float32)
    r = rng.uniform(0.5, reach, n)
    a = rng.uniform(-np.pi, np.pi, n)
    p[:, 0], p[:, 1] = r * np.cos(a), r * np.sin(a)
    p[:, 2] = rng.uniform(-2.0, 6.0, n) * (1 + np.sin(3 * a + seed))
    p[:, 3] = 1
    return p


def rotate_sectors(cloud, sectors):
    """the cloud turned about z by `sectors` sectors of 6 degrees"""
    th = np.deg2rad(6.0 * sectors)
    out = cloud.copy()
    out[:, 0] = np.cos(th) * cloud[:, 0] - np.sin(th) * cloud[:, 1]
    out[:, 1] = np.sin(th) * cloud[:, 0] + np.cos(th) * cloud[:, 1]
    return out


def pair_table(orc):
    """(dist, shift) of every ordered pair (q, i), i < q - num_exclude_recent, as a dict: computed once, shared by the callers"""
    tab = {}
    for q in range(len(orc.polar)):
        for i in range(max(0, q - orc.excl)):
            tab[q, i] = orc.distance(q, i)
    return tab


def rank(orc, first, count, k, table=None):
    """-> (idx int64, dist float64, shift int32), each (count, k)"""
    idx = np.full((count, k), -1, np.int64)
    dist = np.full((count, k), DBL_MAX, np.float64)
    shift = np.zeros((count, k), np.int32)
    for row in range(count):
        q = first + row
        cand = []
        for i in range(max(0, q - orc.excl)):
            d, s = table[q, i] if table is not None else orc.distance(q, i)
            cand.append((d, i, s))
        cand.sort(key=lambda c: (c[0], c[1]))
        for r, (d, i, s) in enumerate(cand[:k]):
            idx[row, r], dist[row, r], shift[row, r] = i, d, s
    return idx, dist, shift


def shift_yaw(shift):
    """trans::deg2rad<float>(6 degrees * shift), as ScanContextOracle.query forms it"""
    return np.float32(float(np.float32(np.float32(360.0) / np.float32(60.0)) * np.float32(shift)) * np.pi / 180.0)


def find_loops(orc, first, count, table=None):
    """-> [(id, match or -1, yaw float32, min_dist or None)]: the k = 1 ranking under query's threshold (ScanContext.cpp:273, strict)"""
    idx, dist, shift = rank(orc, first, count, 1, table)
    out = []
    for row in range(count):
        i, d, s = int(idx[row, 0]), float(dist[row, 0]), int(shift[row, 0])
        if i < 0:
            out.append((first + row, -1, np.float32(0), None))
        elif d > float(orc.dist_thres):
            out.append((first + row, -1, np.float32(0), d))
        else:
            out.append((first + row, i, shift_yaw(s), d))
    return out
