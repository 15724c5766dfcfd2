"""The liorf method at the bench's headline shape -- a 65 536-point 64-beam scan against a 1 M-point map, both in HBM -- next to LOAM in the
same process on the same clouds and initial guesses, through pcr_scan2map (index rebuilt per call) and pcr_set_target + pcr_align.  LOAM runs
with the reference's own constants (8 iterations, early exit), liorf with the file's (30 iterations at most, its convergence test).
Prints one JSON line per (method, entry point):
  ms_per_call      median over --reps rounds of the mean wall time of a call over the scans of a round (host clock, stream drained)
  iterations       mean linearisations per call
  call_us_per_launch   ms_per_call / (iterations + 1) -- a launch per linearisation and the one that ends the loop: the host time of the
                       whole call spread over its launches (not the duration of a launch: it carries the call's fixed costs)
  ratio_to_loam    ms_per_call / LOAM's of the same run
The two methods alternate call by call inside every round, after a warm-up round that is not timed.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleslam_amd import LiorfRegister, LoamRegister, synth  # noqa: E402

SEED = 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    world, map_np = synth.make_map(args.map_points, seed=SEED + 2)
    scans, inits = [], []
    for k in range(args.scans):
        s, T = synth.make_scan(world, k, seed=SEED + 2)
        scans.append(torch.from_numpy(s).cuda())
        inits.append(synth.perturb(T, SEED + 2 + k))
    d_map = torch.from_numpy(map_np).cuda()
    regs = {"loam": LoamRegister(), "liorf": LiorfRegister()}
    times = {(m, e): [] for m in regs for e in ("scan2map", "align")}
    iters = {(m, e): [] for m in regs for e in ("scan2map", "align")}
    for entry in ("scan2map", "align"):
        if entry == "align":
            for r in regs.values():
                r.setTarget(d_map)
        for rep in range(args.reps + 1):      # round 0 warms up
            acc = {m: 0.0 for m in regs}
            its = {m: 0 for m in regs}
            for k in range(args.scans):
                for m, r in regs.items():      # the methods alternate call by call
                    pose = inits[k].copy()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if entry == "scan2map":
                        r.scan2Map(scans[k], d_map, pose)
                    else:
                        r.align(scans[k], pose)
                    torch.cuda.synchronize()
                    acc[m] += time.perf_counter() - t0
                    its[m] += r.stats()["iterations"]
            if rep:
                for m in regs:
                    times[(m, entry)].append(acc[m] / args.scans * 1e3)
                    iters[(m, entry)].append(its[m] / args.scans)
    for entry in ("scan2map", "align"):
        base = float(np.median(times[("loam", entry)]))
        for m in regs:
            ms = float(np.median(times[(m, entry)]))
            it = float(np.mean(iters[(m, entry)]))
            row = dict(method=m, entry=entry, ms_per_call=ms, ms_min=float(np.min(times[(m, entry)])), ms_max=float(np.max(times[(m, entry)])),
                       iterations=it, ratio_to_loam=ms / base, scan_points=int(scans[0].shape[0]), map_points=int(args.map_points))
            row["call_us_per_launch"] = ms * 1e3 / (it + 1.0)
            print(json.dumps(row))


if __name__ == "__main__":
    main()
