"""gicp beside vgicp at the headline shape: a 65 536-point scan against a 1 M-point map, reference defaults, device-resident clouds.
Prints one JSON line per method:
  scan2map_ms   pcr_scan2map_device, the target's index and covariances rebuilt by every call (host clock around the call)
  align_ms      pcr_align against the target kept by pcr_set_target
  pass_us       the mean pass of a scan2map call: pcr_stats.solve_ms over the passes the device loop evaluated (events on the handle's stream)
  index_ms      pcr_stats.index_ms of a scan2map call: the target's preparation
  d_truth       the final pose against the scene's true pose (m, rad); gicp's line adds d_vgicp
Medians of --reps calls after --warmup calls, with the smallest and the largest beside them.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleslam_amd import make_register, synth  # noqa: E402


def _spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regularization", type=int, default=3, help="pcr_params.vgicp_regularization (PCR_REG_*: 0 NONE .. 4 FROBENIUS; default 3 PLANE), both methods")
    ap.add_argument("--voxel-mode", type=int, default=0, help="pcr_params.vgicp_voxel_mode (PCR_VOXEL_*: 0 ADDITIVE, 1 ADDITIVE_WEIGHTED, 2 MULTIPLICATIVE), vgicp")
    ap.add_argument("--calls", type=int, default=0, help="only this many gicp scan2map calls, nothing printed (for a kernel trace)")
    a = ap.parse_args()
    world, m = synth.make_map(a.map_points, seed=20261003)
    scan, T = synth.make_scan(world, 0, seed=20261003)
    init = synth.perturb(T, 20261003)
    d_map, d_scan = torch.from_numpy(m).cuda(), torch.from_numpy(scan).cuda()
    if a.calls:
        reg = make_register("gicp")
        for _ in range(a.calls):
            reg.scan2Map(d_scan, d_map, init.copy())
        return
    poses = {}
    for method in ("vgicp", "gicp"):
        reg = make_register(method, vgicp_regularization=a.regularization, vgicp_voxel_mode=a.voxel_mode)
        s2m, ali, idx, pas = [], [], [], []
        for k in range(a.warmup + a.reps):
            pose = init.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg.scan2Map(d_scan, d_map, pose)
            dt = time.perf_counter() - t0
            st = reg.stats()
            if k >= a.warmup:
                s2m.append(dt * 1e3); idx.append(st["index_ms"]); pas.append(st["solve_ms"] * 1e3 / max(st["attempts"], 1))
        reg.setTarget(d_map)
        for k in range(a.warmup + a.reps):
            pose = init.copy()
            t0 = time.perf_counter()
            conv = reg.align(d_scan, pose)
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                ali.append(dt * 1e3)
        poses[method] = pose
        row = dict(method=method, regularization=a.regularization, voxel_mode=a.voxel_mode, n_src=int(scan.shape[0]), n_dst=int(m.shape[0]), converged=bool(conv), iterations=st["iterations"], passes=st["attempts"],
                   scan2map_ms=_spread(s2m), index_ms=_spread(idx), pass_us=_spread(pas), align_ms=_spread(ali),
                   d_truth=[float("%.3g" % v) for v in synth.pose_error(pose, T)])
        if method == "gicp":
            row["d_vgicp"] = [float("%.3g" % v) for v in synth.pose_error(pose, poses["vgicp"])]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
