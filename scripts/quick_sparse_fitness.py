"""Times of the fitness scores on the sparse target index (csrc/sparse_fitness.hip) against the dense index of the same run:
    python scripts/quick_sparse_fitness.py [--points 1000000] [--scan 65536] [--calls 30] [--out FILE.json]
1. A compact synthetic map the dense table holds and a scan of --scan points at the truth (HBM-resident): pcr_fitness_gated under AUTO (the dense
   kernel) and under SPARSE, at a gate of 1 m^2 and ungated, and pcr_relocalize's default window (1053 hypotheses on 4096 points, the refinements,
   the final score) both ways.
2. A two-session map (the map and its copy 30 km / 20 km / 8 km away, half of --points each): pcr_fitness_gated in the near and the far copy
   under AUTO -- where the dense index answers, that alone; where it refuses, the dense launch and then the sparse one -- and under SPARSE.
3. The one-off build of the sparse index: the first score after a pcr_set_target less the median of the scores after it.
Per operation the median and the quartiles of `calls` host-clock times around the call (every call ends in a device synchronise).  Scores of the two
indices are compared for equality before anything is timed.  Prints one JSON line; needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

DBL_MAX = float(np.finfo(np.float64).max)


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


def scores(reg, scan, pose, calls):
    out = {}
    for name, gate in (("gate_1", 1.0), ("ungated", DBL_MAX)):
        out[name] = timed(lambda: reg.fitnessGated(scan, pose, gate), calls)
        out[name]["answer"] = list(reg.fitnessGated(scan, pose, gate))
        out[name]["index"] = reg.queryIndexInfo()["kind"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--scan", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from simpleslam_amd import LoamRegister, synth
    from simpleslam_amd.pcr import QUERY_INDEX_SPARSE

    res = dict(points=a.points, scan=a.scan, calls=a.calls)
    world, m = synth.make_map(a.points, seed=5)
    scan, T = synth.make_scan(world, 0, seed=5, beams=64, azimuths=max(a.scan // 64, 1))
    scan = np.ascontiguousarray(scan[:a.scan])
    res["scan_points"] = len(scan)
    d_scan = torch.from_numpy(scan).cuda()
    pose = synth.perturb(T, 5, trans=0.1, rot_deg=0.5)
    dense, sparse = LoamRegister(), LoamRegister(query_index=QUERY_INDEX_SPARSE)
    dense.setTarget(m); sparse.setTarget(m)
    for gate in (1.0, DBL_MAX):
        assert dense.fitnessGated(d_scan, pose, gate) == sparse.fitnessGated(d_scan, pose, gate), "the two indices disagree"
    res["compact"] = dict(dense=scores(dense, d_scan, pose, a.calls), sparse=scores(sparse, d_scan, pose, a.calls))
    res["compact"]["ratio_sparse_over_dense"] = {g: res["compact"]["sparse"][g]["median_ms"] / res["compact"]["dense"][g]["median_ms"] for g in ("gate_1", "ungated")}

    def reloc(reg):
        p = pose.copy()
        p[:3, 3] += (0.8, -0.6, 0.0)
        return reg.relocalize(d_scan, p)
    ra, rb = reloc(dense), reloc(sparse)
    assert ra[2] == rb[2] and [c["score"] for c in ra[1]] == [c["score"] for c in rb[1]], "relocalisation differs between the indices"
    res["relocalize_default_window"] = dict(dense=timed(lambda: reloc(dense), max(a.calls // 3, 3)), sparse=timed(lambda: reloc(sparse), max(a.calls // 3, 3)))

    ts = []
    for _ in range(max(a.calls // 3, 3)):      # the build: the first score after a setTarget less a score after it
        sparse.setTarget(m)
        t0 = time.perf_counter()
        sparse.fitnessGated(d_scan, pose, 1.0)
        t1 = time.perf_counter()
        sparse.fitnessGated(d_scan, pose, 1.0)
        ts.append((t1 - t0) - (time.perf_counter() - t1))
    res["sparse_index_build"] = quartiles(ts)

    half = m[::2].copy()
    off = np.array([30000.0, 20000.0, 8000.0], np.float32)
    far = half.copy(); far[:, :3] += off
    both = np.ascontiguousarray(np.vstack([half, far]))
    there = pose.copy(); there[:3, 3] += off
    auto, sp = LoamRegister(), LoamRegister(query_index=QUERY_INDEX_SPARSE)
    auto.setTarget(both); sp.setTarget(both)
    two = {}
    for where, P in (("near_copy", pose), ("far_copy", there)):
        for gate in (1.0, DBL_MAX):
            assert auto.fitnessGated(d_scan, P, gate) == sp.fitnessGated(d_scan, P, gate), "AUTO and SPARSE disagree on the two-session map"
        two[where] = dict(auto=scores(auto, d_scan, P, a.calls), sparse=scores(sp, d_scan, P, a.calls))
    res["two_sessions"] = two
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
