"""VGICP's neighbourhood settings side by side: pcr_params.vgicp_search = DIRECT1, DIRECT7, DIRECT27 on a 65 536-point scan against a 1 M-point
map (synth.make_map, spacing 0.22), device-resident clouds.  One JSON line per setting:
  scan2map_ms     pcr_scan2map, the target prepared by every call (host clock around the call)
  solve_pass_us   pcr_stats.solve_ms of a scan2map call over the passes its device loop evaluated (events on the handle's stream)
  lin_us          one linearisation at the initial pose on the kept target (pcr_vgicp_linearize: the source's covariances, one
                  vgicp_linearize_kernel<false>, the fold, the read-back of the slots): host clock around the call MINUS the same call on a
                  one-point scan, so what is left is the scan's covariances and the pass
  pairs_per_point pcr_vgicp_linearize's n_corr over the scan's points
  iterations, passes, d_truth (the final pose against the scene's true pose: m, rad)
Medians of --reps calls after --warmup calls, with the smallest and the largest beside them.  --only N runs one setting (-2: the field never
named, for a build without it; PCR_LIB names the library).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleslam_amd import VgicpRegister, synth  # noqa: E402

SEED = 20261019
NAMES = {0: "DIRECT27", 1: "DIRECT7", 2: "DIRECT1"}


def _spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", type=int, default=-1, help="one setting: 0 DIRECT27, 1 DIRECT7, 2 DIRECT1; -2: the library's default, vgicp_search never named")
    a = ap.parse_args()
    world, m = synth.make_map(a.map_points, seed=SEED, spacing=0.22)
    scan, T = synth.make_scan(world, 0, seed=SEED, beams=a.beams, azimuths=a.azimuths)
    init = synth.perturb(T, SEED, trans=0.1, rot_deg=0.5)
    d_map, d_scan = torch.from_numpy(m).cuda(), torch.from_numpy(scan).cuda()
    d_one = d_scan[:1].contiguous()
    for search in ([2, 1, 0] if a.only == -1 else [a.only]):
        kw = {} if search == -2 else dict(vgicp_search=search)
        reg = VgicpRegister(**kw)
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
        reg.setTarget(d_map)
        full, one, n_pairs = [], [], 0
        for k in range(a.warmup + a.reps):
            for cloud, acc in ((d_scan, full), (d_one, one)):
                t0 = time.perf_counter()
                lin = reg.linearize(cloud, init)
                if k >= a.warmup:
                    acc.append((time.perf_counter() - t0) * 1e6)
                if cloud is d_scan:
                    n_pairs = lin["n"]
        row = dict(vgicp_search=NAMES.get(search, "default"), n_src=int(scan.shape[0]), n_dst=int(m.shape[0]), converged=bool(conv), iterations=its, passes=passes,
                   scan2map_ms=_spread(s2m), solve_pass_us=_spread(sol), lin_us=dict(_spread(np.array(full) - float(np.median(one))), overhead=round(float(np.median(one)), 1)),
                   pairs_per_point=round(n_pairs / scan.shape[0], 3), d_truth=[float("%.3g" % v) for v in synth.pose_error(pose, T)])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
