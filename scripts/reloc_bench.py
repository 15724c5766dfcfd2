"""Relocalisation at the flagship sizes: a 65 536-point scan against a 1 M-point map, LOAM, the default window (+-2 m at 0.5 m,
+-30 deg at 5 deg: K = 1 053 hypotheses, 4 096-point subset).  Prints one JSON line:
  coarse_ms / coarse_qps        pcr_fitness_batch of the K hypotheses on the subset (1-NN queries per second = K x score_points / time)
  single_qps                    pcr_fitness_gated (fitness_kernel) of one pose on all 65 536 points, the same process
  host_loop_ms                  a host loop of pcr_fitness_gated over the same K poses and subset
  refine_ms, total_ms           pcr_align from each candidate's hypothesis pose (sum), the whole pcr_relocalize
Times are medians of --reps runs after one warm-up.  Not part of bench.py."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleslam_amd import LoamRegister, reloc_hypotheses, synth  # noqa: E402


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20261010)
    a = ap.parse_args()
    world, m = synth.make_map(a.map_points, seed=a.seed)
    scan, T = synth.make_scan(world, 0, seed=a.seed)
    d_scan, d_map = torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda()
    reg = LoamRegister()
    reg.setTarget(d_map)
    ang = math.radians(20.0)
    click = T.copy()
    click[:3, :3] = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]]) @ T[:3, :3]
    click[:3, 3] += [1.4, -1.1, 0.0]
    poses = reloc_hypotheses(click)
    K, sp = len(poses), 4096
    coarse_ms = _median_ms(lambda: reg.fitnessBatch(d_scan, poses, 1.0, sp), a.reps)
    single_ms = _median_ms(lambda: reg.fitnessGated(d_scan, T, 1.0), a.reps)
    idx = (np.arange(sp, dtype=np.int64) * len(scan)) // sp
    d_sub = torch.from_numpy(np.ascontiguousarray(scan[idx])).cuda()
    host_loop_ms = _median_ms(lambda: [reg.fitnessGated(d_sub, P, 1.0) for P in poses], max(1, a.reps // 3))
    out = {}

    def reloc():
        p = click.copy()
        out["r"] = reg.relocalize(d_scan, p)
        out["pose"] = p
    total_ms = _median_ms(reloc, a.reps)
    _, cands, chosen = out["r"]

    def refine():
        for c in cands:
            p = poses[c["hypothesis"]].copy()
            reg.align(d_scan, p)
    refine_ms = _median_ms(refine, a.reps)
    et, er = synth.pose_error(out["pose"], T)
    print(json.dumps(dict(
        workload="relocalize loam 65536 x %d" % len(m), K=K, score_points=sp,
        coarse_ms=round(coarse_ms, 4), coarse_qps=K * sp / (coarse_ms * 1e-3),
        single_ms=round(single_ms, 4), single_qps=len(scan) / (single_ms * 1e-3),
        host_loop_ms=round(host_loop_ms, 3), coarse_speedup_vs_host_loop=round(host_loop_ms / coarse_ms, 2),
        refine_ms=round(refine_ms, 4), total_ms=round(total_ms, 4), candidates=len(cands), chosen=chosen,
        chosen_hypothesis=cands[chosen]["hypothesis"], error_m=et, error_deg=math.degrees(er))))


if __name__ == "__main__":
    main()
