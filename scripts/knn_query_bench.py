"""pcr_knn and pcr_radius_search at the flagship sizes: a 1 M-point map kept on a LOAM handle, queried with (a) the 65 536 points of a
scan at its true pose and (b) 65 536 of the map's own points, for k in {1, 5, 20, 32} and r in {0.5, 2.0} (sorted).  Prints one JSON
line per row:
  device_ns_per_query   from two events on the handle's stream around the call: the kernels and the copy of the results to the host
  call_ns_per_query     host clock around the call
  ref_ns_per_query      the reference's nanoflann on the same cloud, its queries split over --threads CPU threads (oracle/_ref; the tree
                        is built once and not timed).  k-NN: ref_kd_knn_batch per slice.  Radius: one call per query through ctypes
                        on --ref-queries of the queries (a few microseconds of call overhead per query are in that figure).
Medians of --reps runs after a warm-up run.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import oracle  # noqa: E402
from simpleslam_amd import LoamRegister, synth  # noqa: E402


def _timed(fn, stream, reps):
    fn()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        stream.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(dev)), float(np.median(wall))


def _ref_knn_s(R, tree, q, k, threads, reps):
    parts = [np.ascontiguousarray(p) for p in np.array_split(q, threads)]
    outs = [(np.zeros((len(p), k), np.int64), np.zeros((len(p), k))) for p in parts]

    def one(j):
        p, (i, d) = parts[j], outs[j]
        R.ref_kd_knn_batch(tree, p.ctypes.data_as(C.c_void_p), len(p), p.shape[1], k, i.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    ts = []
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            list(ex.map(one, range(len(parts))))
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:]))


def _ref_radius_s(R, tree, q, r, threads, reps, n_map):
    q64 = np.ascontiguousarray(q[:, :3].astype(np.float64))
    parts = np.array_split(np.arange(len(q64)), threads)
    bufs = [(np.zeros(n_map, np.uint64), np.zeros(n_map)) for _ in parts]
    counts = np.zeros(len(q64), np.int64)

    def one(j):
        i, d = bufs[j]
        ip, dp = i.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
        for t in parts[j]:
            counts[t] = R.ref_kd_radius(tree, q64[t].ctypes.data_as(C.c_void_p), float(r), 1, ip, dp, n_map)
    ts = []
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            list(ex.map(one, range(len(parts))))
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), float(counts.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=65_536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ref-queries", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=20261010)
    a = ap.parse_args()
    world, m = synth.make_map(a.map_points, seed=a.seed)
    scan, T = synth.make_scan(world, 0, seed=a.seed)
    Tf = T.astype(np.float32)
    qs = np.zeros((len(scan), 4), np.float32)
    qs[:, :3] = scan[:, :3] @ Tf[:3, :3].T + Tf[:3, 3]
    qs = np.ascontiguousarray(qs[:a.queries])
    rng = np.random.default_rng(a.seed)
    qm = np.ascontiguousarray(m[rng.choice(len(m), min(a.queries, len(m)), replace=False)])
    stream = torch.cuda.Stream()
    reg = LoamRegister()
    reg.set_stream(stream.cuda_stream)
    reg.setTarget(torch.from_numpy(m).cuda())
    have_ref = oracle.ref_available()
    R = tree = None
    if have_ref:
        R = oracle.ref_lib()
        m32 = np.ascontiguousarray(m, np.float32)
        tree = R.ref_kd_build(m32.ctypes.data_as(C.c_void_p), m32.shape[0], m32.shape[1])
    for name, q in (("scan", qs), ("map", qm)):
        d_q = torch.from_numpy(q).cuda()
        for k in (1, 5, 20, 32):
            dev, wall = _timed(lambda: reg.knn(d_q, k), stream, a.reps)
            row = dict(op="knn", queries=name, n_q=len(q), k=k, device_ns_per_query=round(dev / len(q) * 1e9, 2), call_ns_per_query=round(wall / len(q) * 1e9, 2))
            if have_ref:
                row["ref_ns_per_query"] = round(_ref_knn_s(R, tree, q, k, a.threads, 2) / len(q) * 1e9, 2)
                row["ref_threads"] = a.threads
            print(json.dumps(row), flush=True)
        for r in (0.5, 2.0):
            out = {}

            def run():
                out["o"] = reg.radiusSearch(d_q, r, sorted=True)
            dev, wall = _timed(run, stream, a.reps)
            row = dict(op="radius", queries=name, n_q=len(q), r=r, mean_count=round(len(out["o"][1]) / len(q), 2),
                       device_ns_per_query=round(dev / len(q) * 1e9, 2), call_ns_per_query=round(wall / len(q) * 1e9, 2))
            if have_ref:
                s, mc = _ref_radius_s(R, tree, q[:a.ref_queries], r, a.threads, 1, len(m))
                row["ref_ns_per_query"] = round(s / min(len(q), a.ref_queries) * 1e9, 2)
                row["ref_mean_count"] = round(mc, 2)
                row["ref_threads"] = a.threads
            print(json.dumps(row), flush=True)
    if tree:
        R.ref_kd_free(tree)


if __name__ == "__main__":
    main()
