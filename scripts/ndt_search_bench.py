"""NDT's neighbourhood settings side by side: pcr_params.ndt_search = DIRECT1, DIRECT7, DIRECT26 on a 65 536-point scan against the 5 M-point
map of BASELINE config 5 (bench.py --method ndt: same map, same seed), device-resident clouds.  One JSON line per setting:
  scan2map_ms   pcr_scan2map_device, the target rebuilt by every call (host clock around the call)
  pass_us       one pass of each kind at the initial pose, by the launches of the device-resident loop (pcr_ndt_pass_sums: kind 0 =
                derivatives with the float Hessian, 1 = the line search's 7-component pass, 2 = computeHessian): host clock around the
                call MINUS the same call on a one-point scan (its launches, copy and round trip), so what is left is the pass itself
  solve_pass_us pcr_stats.solve_ms of a scan2map call over the passes its device loop evaluated (events on the handle's stream)
  iterations, passes
  pairs_per_point_call   (point, voxel) pairs of one profiled scan2map per scan point, all its derivative passes together:
                (pairs_grad + pairs_hess) / n_src, with the two counters (gradient-only passes / passes with the float Hessian; the
                computeHessian passes count none) and the call's passes and iterations beside it.  One pass's share is a counter over
                n_src over the number of passes of its kind -- an integer that the counters give away (profiles/ndt_search_notes.md)
  d_truth       the final pose against the scene's true pose (m, rad)
Medians of --reps calls after --warmup calls, with the smallest and the largest beside them.  --only N runs one setting (for A/B runs of
two builds: PCR_LIB names the library).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleslam_amd import NdtRegister, synth  # noqa: E402

SEED = 20261003 + 5      # bench.py: SEED + cfg, BASELINE config 5
NAMES = {1: "DIRECT26", 2: "DIRECT7", 3: "DIRECT1"}


def _spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=5_000_000)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, default=-1, help="one setting: 1 DIRECT26, 2 DIRECT7, 3 DIRECT1; -2: the library's default, ndt_search never named (a build without the field)")
    a = ap.parse_args()
    world, m = synth.make_map(a.map_points, seed=SEED, spacing=0.22)
    scan, T = synth.make_scan(world, 0, seed=SEED, beams=a.beams, azimuths=a.azimuths)
    init = synth.perturb(T, SEED, trans=0.1, rot_deg=0.5)
    p6 = np.concatenate([init[:3, 3], np.zeros(3)])
    d_map, d_scan = torch.from_numpy(m).cuda(), torch.from_numpy(scan).cuda()
    d_one = d_scan[:1].contiguous()
    for search in ([3, 2, 1] if a.only == -1 else [a.only]):
        kw = {} if search == -2 else dict(ndt_search=search)
        reg = NdtRegister(**kw)
        s2m, sol = [], []
        for k in range(a.warmup + a.reps):
            pose = init.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            conv = reg.scan2Map(d_scan, d_map, pose)
            dt = time.perf_counter() - t0
            st = reg.stats()
            if k >= a.warmup:
                s2m.append(dt * 1e3); sol.append(st["solve_ms"] * 1e3 / max(st["attempts"], 1))
        its, passes = st["iterations"], st["attempts"]
        prof = NdtRegister(**kw)
        prof.set_profile(2)
        prof.scan2Map(d_scan, d_map, init.copy())
        ps = prof.stats()
        reg.setTarget(d_map)
        pass_us = {}
        for kind in (0, 1, 2):
            full, one = [], []
            for k in range(a.warmup + a.reps):
                for cloud, acc in ((d_scan, full), (d_one, one)):
                    t0 = time.perf_counter()
                    reg.derivatives(cloud, p6, device_loop=True, kind=kind)
                    if k >= a.warmup:
                        acc.append((time.perf_counter() - t0) * 1e6)
            pass_us[str(kind)] = dict(_spread(np.array(full) - float(np.median(one))), overhead=round(float(np.median(one)), 1))
        row = dict(ndt_search=NAMES.get(search, "default"), n_src=int(scan.shape[0]), n_dst=int(m.shape[0]), converged=bool(conv), iterations=its, passes=passes,
                   scan2map_ms=_spread(s2m), solve_pass_us=_spread(sol), pass_us=pass_us,
                   pairs_per_point_call=round((ps["pairs_grad"] + ps["pairs_hess"]) / scan.shape[0], 3), pairs_grad=ps["pairs_grad"], pairs_hess=ps["pairs_hess"], profiled_passes=ps["attempts"], profiled_iterations=ps["iterations"],
                   d_truth=[float("%.3g" % v) for v in synth.pose_error(pose, T)])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
