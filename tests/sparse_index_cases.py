"""Clouds and queries of the sparse target index's tests (test_sparse_index_host.py on the CPU, test_sparse_index_gpu.py on the device)."""
import numpy as np


def cloud(xyz):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = np.asarray(xyz, np.float32).reshape(-1, 3)
    return out


def cluster(n, centre, seed, spread=(4.0, 4.0, 1.0)):
    rng = np.random.default_rng(seed)
    return (np.asarray(centre, np.float64) + rng.normal(0.0, 1.0, (n, 3)) * np.asarray(spread)).astype(np.float32)


def two_clusters(n=300, seed=0, gap=(30000.0, 20000.0, 8000.0), spread=(4.0, 4.0, 1.0)):
    """two clusters of n points, 30 km / 20 km / 8 km apart: 4.8e12 cells of 1 m, no dense table holds them"""
    return cloud(np.vstack([cluster(n, (12.0, -7.0, 1.5), seed, spread), cluster(n, np.asarray(gap) + (12.0, -7.0, 1.5), seed + 1, spread)]))


def stray(n=600, seed=3, at=4.0e6):
    """a cluster and one stray return at 4e6 m: 4e6 x ~30 x 4e6 cells"""
    xyz = cluster(n, (0.0, 0.0, 0.0), seed)
    xyz[n // 2] = (at, 3.0, -at)
    return cloud(xyz)


def edge_cloud(n, seed=0):
    """n points around the origin: cell faces, negative coordinates, exact duplicates and exact distance ties among them"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform((-6.0, -6.0, -2.0), (6.0, 6.0, 2.0), (n, 3)).astype(np.float32)
    m = n // 4
    xyz[:m] = np.round(xyz[:m])                     # on cell faces (1 m cells), negative ones too; many exact duplicates and ties
    if n >= 8:
        xyz[n - 3:] = xyz[:3]                       # exact duplicates far apart in row order
    return cloud(xyz)


def queries_for(target, seed=0, n_in=24):
    """inside the clusters, halfway between the extremes, outside the box, on lattice points (ties), and rows that are not finite"""
    t = target[np.isfinite(target[:, :3]).all(axis=1), :3].astype(np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = t.min(axis=0), t.max(axis=0)
    q = [t[rng.integers(0, len(t), n_in)] + rng.normal(0.0, 0.3, (n_in, 3)),       # inside
         np.round(t[rng.integers(0, len(t), 8)]),                                    # lattice points: ties
         t[:2],                                                                       # a target point itself
         [0.5 * (lo + hi)],                                                           # halfway
         [hi + (15000.0, 40.0, 3.0), lo - (7.0, 15000.0, 0.0), hi + 2.5, lo - 0.5, (lo[0] - 500.0, hi[1] + 500.0, 0.5 * (lo[2] + hi[2]))],
         [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)]]
    return cloud(np.vstack([np.asarray(x, np.float64).reshape(-1, 3) for x in q]))
