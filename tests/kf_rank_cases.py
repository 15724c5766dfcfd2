"""Shared by tests/test_kf_rank_host.py and tests/test_kf_rank_gpu.py: the brute force that defines the key-frame ranking by distance, in
numpy with the library's rounding order, and the small cases both tests run."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def brute(xyz, first, count, excl, radius, k):
    """For every query q of [first, first + count): candidates [0, q - excl) with finite coordinates on both sides and
    (dx*dx + dy*dy) + dz*dz <= radius*radius, each operation rounded on its own (numpy's elementwise float64), the k best by (d2, index)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        r2 = np.float64(radius) * np.float64(radius)
    idx = np.full((count, k), -1, np.int64)
    d2 = np.full((count, k), DBL_MAX)
    for q in range(first, first + count):
        lim = q - excl
        if lim <= 0 or not np.isfinite(xyz[q]).all():
            continue
        c = xyz[:lim]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = c[:, 0] - xyz[q, 0], c[:, 1] - xyz[q, 1], c[:, 2] - xyz[q, 2]
            d = (dx * dx + dy * dy) + dz * dz
            ok = np.isfinite(c).all(axis=1) & (d <= r2)
        cand = np.nonzero(ok)[0]
        best = cand[np.lexsort((cand, d[cand]))][:k]
        idx[q - first, :best.size] = best
        d2[q - first, :best.size] = d[best]
    return idx, d2


def _rng_points(n, seed, scale=4.0):
    return np.random.default_rng(seed).uniform(-scale, scale, (n, 3))


def small_cases():
    """-> list of (name, xyz (n, 3), num_exclude_recent, radius); every case is run over the window [0, n) at k = 1 and k = 8."""
    ulp25 = 2.0 ** -24      # (2^-24)^2 = 2^-48 = the spacing of doubles at 25: d2 = nextafter(25, inf) exactly
    cases = [
        ("one key frame", [[1.0, 2.0, 3.0]], 0, 10.0),
        ("n equals the exclusion", _rng_points(3, 1), 3, 100.0),
        ("n is the exclusion plus one", _rng_points(4, 2), 3, 100.0),
        ("n is the exclusion plus two: the first query with one candidate", _rng_points(5, 2), 3, 100.0),
        ("fewer than k in range", _rng_points(12, 3), 0, 3.0),
        ("duplicate positions", [[0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1]], 0, 5.0),
        ("mirrored about the query", [[3, 0, 0], [-3, 0, 0], [0, 3, 0], [0, -3, 0], [0, 0, 3], [0, 0, -3], [1, 2, 2], [-1, -2, -2], [0, 0, 0]], 0, 4.0),
        ("small integers", np.random.default_rng(4).integers(-3, 4, (40, 3)).astype(float), 1, 4.0),
        ("d2 equals radius^2 is in, the next double above is out", [[3, 4, 0], [5, 0, ulp25], [0, 5, 0], [5, 0, -ulp25], [0, 0, 0]], 0, 5.0),
        ("radius 0 with a duplicate", [[1.5, -2.5, 0.25], [1.5, -2.5, 0.5], [1.5, -2.5, 0.25]], 0, 0.0),
        ("a NaN and an Inf as candidates", [[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 0, 0], [0, 0, -np.inf], [0.5, 0, 0]], 0, 10.0),
        ("a NaN and an Inf as queries", [[0, 0, 0], [1, 0, 0], [0, np.nan, 0], [2, 0, 0], [np.inf, 0, 0], [3, 0, 0]], 0, 10.0),
        ("an Inf under a radius whose square overflows", [[0, 0, 0], [np.inf, 0, 0], [1, 0, 0], [2, 0, 0]], 0, 1e200),
    ]
    return [(name, np.asarray(xyz, dtype=np.float64).reshape(-1, 3), excl, radius) for name, xyz, excl, radius in cases]


def random_walk(n, seed, step=1.0):
    """A walk round a closed course, lap after lap with a little noise: it revisits itself every 200 steps."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / 200.0
    r = 200.0 * step / (2.0 * np.pi)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), 0.05 * np.sin(3 * a)], axis=1)
    return xyz + rng.normal(0.0, 0.3, xyz.shape)


# what both entry points refuse: (name, dict of arguments changed from a valid call on 6 key frames)
REFUSALS = [
    ("k is 0", dict(k=0)),
    ("k is 9", dict(k=9)),
    ("radius is negative", dict(radius=-1.0)),
    ("radius is NaN", dict(radius=float("nan"))),
    ("radius is Inf", dict(radius=float("inf"))),
    ("num_exclude_recent is negative", dict(excl=-1)),
    ("first + count exceeds n", dict(first=2, count=5)),
    ("idx is NULL", dict(null="idx")),
    ("d2 is NULL", dict(null="d2")),
]
