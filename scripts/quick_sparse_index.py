"""Times of the sparse target index (csrc/sparse_index.hip) against the dense index of the same run and the same cloud:
    python scripts/quick_sparse_index.py [--points 1000000] [--queries 65536] [--calls 30] [--out FILE.json]
A synthetic map that the dense table holds (HBM-resident queries), then the two-cluster cloud that only the sparse index answers (queries
inside the clusters; 64 queries halfway between them apart).  Per
operation -- the build of the sparse index, pcr_knn at k = 1, 5 and 20, pcr_radius_search at 1 m (sorted) -- the median and the quartiles of
`calls` host-clock times around the call (every call ends in a device synchronise and the copy of its results to the host, on both
indices alike), and the ratio sparse / dense of the medians.  The build is timed as the first query after a pcr_set_target less the median
of the queries after it.  Prints one JSON line; needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def quartiles(ts):
    a = np.sort(np.asarray(ts)) * 1e3
    return dict(median_ms=float(np.median(a)), q1_ms=float(np.percentile(a, 25)), q3_ms=float(np.percentile(a, 75)), min_ms=float(a[0]), calls=len(a))


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return quartiles(ts)


def measure(reg, q, calls):
    out = {}
    for k in (1, 5, 20):
        out[f"knn_k{k}"] = timed(lambda: reg.knn(q, k), calls)
    out["radius_1m"] = timed(lambda: reg.radiusSearch(q, 1.0, sorted=True), calls)
    return out


def build_times(reg, target, q1, calls):
    """the first query after a setTarget builds the index; the ones after it do not"""
    ts = []
    for _ in range(calls):
        reg.setTarget(target)
        t0 = time.perf_counter()
        reg.knn(q1, 1)
        t1 = time.perf_counter()
        reg.knn(q1, 1)
        ts.append((t1 - t0) - (time.perf_counter() - t1))
    return quartiles(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import sparse_index_cases as cases
    from simpleslam_amd import LoamRegister, synth
    from simpleslam_amd.pcr import QUERY_INDEX_SPARSE

    _, m = synth.make_map(a.points, seed=5)
    rng = np.random.default_rng(1)
    q = np.ascontiguousarray(m[rng.choice(len(m), a.queries, replace=a.queries > len(m))])
    q[:, :3] += rng.normal(0.0, 0.1, (a.queries, 3)).astype(np.float32)
    qd = torch.from_numpy(q).cuda()
    res = dict(points=a.points, queries=a.queries, calls=a.calls)
    dense, sparse = LoamRegister(), LoamRegister(query_index=QUERY_INDEX_SPARSE)
    dense.setTarget(m); sparse.setTarget(m)
    i_d, d_d = dense.knn(qd, 5)
    i_s, d_s = sparse.knn(qd, 5)
    assert i_d.tobytes() == i_s.tobytes() and d_d.tobytes() == d_s.tobytes(), "the two indices disagree"
    res["dense"] = measure(dense, qd, a.calls)
    res["sparse"] = measure(sparse, qd, a.calls)
    res["dense"]["info"], res["sparse"]["info"] = dense.queryIndexInfo(), sparse.queryIndexInfo()
    res["ratio_sparse_over_dense"] = {k: res["sparse"][k]["median_ms"] / res["dense"][k]["median_ms"] for k in ("knn_k1", "knn_k5", "knn_k20", "radius_1m")}
    res["sparse"]["build"] = build_times(sparse, m, qd[:64], a.calls)
    two = cases.two_clusters(n=a.points // 2, seed=2, spread=(60.0, 60.0, 3.0))
    far = LoamRegister()
    far.setTarget(two)
    q2 = np.ascontiguousarray(two[rng.choice(len(two), a.queries, replace=a.queries > len(two))])
    q2[:, :3] += rng.normal(0.0, 0.1, (a.queries, 3)).astype(np.float32)
    q2d = torch.from_numpy(q2).cuda()
    res["two_clusters"] = measure(far, q2d, a.calls)
    res["two_clusters"]["info"] = far.queryIndexInfo()
    # 64 queries around the point halfway between the clusters, 18 km from either: each scans the rows of both
    mid = np.zeros((64, 4), np.float32)
    mid[:, :3] = 0.5 * (two[0, :3] + two[-1, :3]) + rng.normal(0.0, 50.0, (64, 3)).astype(np.float32)
    res["two_clusters_halfway_64_queries"] = dict(knn_k5=timed(lambda: far.knn(mid, 5), max(a.calls // 6, 3)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
