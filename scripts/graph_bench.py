"""pcr_graph_optimize on the GPU at the ScanContext work's store sizes (profiles/graph_notes.md).

For every size two graphs: an odometry tree with closest-key-frame edges in which 0.5 % of the poses carry a loop edge, and one loop that
spans the whole trajectory (the adversarial case of a block-diagonal preconditioner: information moves one edge per PCG iteration).
Reports LM iterations, PCG iterations, microseconds per PCG iteration, milliseconds in all, and what the caller's alternative costs for the
same poses as far as it exists here: both host copies plus pcr_map_set_poses (there is no CPU solver in the image to race).

usage: python scripts/graph_bench.py [--sizes 1000,5000,20000] [--cases 'tree+loops,one long loop'] [--pcg-cap 4000] [--json out.json]
                                    [--preconditioner block_jacobi|tree] [--repeat 1] [--free-last W]

--free-last W fixes every pose but the last W before optimising (pcr_graph_set_fixed; profiles/graph_fixed_notes.md): what a key-frame event
costs with a window."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import graph_ref as gr                                                     # noqa: E402
from simpleslam_amd import PoseGraph, SubMap                               # noqa: E402


def trajectory(n):
    """a boustrophedon over a field (lanes 200 key frames long, 8 m apart, a key frame per metre) that ends next to where it began"""
    out = []
    lane = 200
    for k in range(n):
        row, col = divmod(k, lane)
        x = col if row % 2 == 0 else lane - 1 - col
        yaw = 0.0 if row % 2 == 0 else np.pi
        T = gr.exp(np.array([0.0, 0.0, yaw, 0.0, 0.0, 0.0]))
        T[:3, 3] = (x, 8.0 * row, 0.0)
        out.append(T)
    return out


def build(n, kind, seed=1):
    rng = np.random.default_rng(seed)
    truth = trajectory(n)
    # dead reckoning: every measurement carries a small error, and the estimates chain them
    meas, est = [], [truth[0]]
    for k in range(1, n):
        Z = gr.inv(truth[k - 1]) @ truth[k] @ gr.exp(np.concatenate([rng.normal(size=3) * 2e-4, rng.normal(size=3) * 2e-3]))
        meas.append(Z)
        est.append(est[-1] @ Z)
    pg = PoseGraph(device=0)
    pg.addPoses(np.stack(est))
    pg.addPrior(truth[0])
    for k in range(1, n):
        pg.addBetween(k - 1, k, meas[k - 1])
    if kind == "tree+loops":
        m = max(1, n // 200)
        ends = rng.choice(np.arange(n // 2, n), size=m, replace=False)
        loops = [(int(rng.integers(0, e // 2)), int(e)) for e in ends]
    else:
        loops = [(0, n - 1)]
    for a, b in loops:
        pg.addLC(a, b, gr.inv(truth[a]) @ truth[b])
    return pg, len(loops)


def alternative_ms(pg, n):
    """poses to the host, poses back through pcr_map_set_poses (the solve itself has no counterpart here)"""
    m = SubMap(device=0)
    pts = np.zeros((4, 4), np.float32)
    for k in range(n):
        m.addKeyFrame(pts, np.eye(4))
    t0 = time.perf_counter()
    P = pg.poses()
    t1 = time.perf_counter()
    m.setPoses(0, P)
    t2 = time.perf_counter()
    pg.applyTo(m)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000,20000")
    ap.add_argument("--pcg-cap", type=int, default=4000, help="pcg_max_iterations of the timed runs (the default rule, 10 x poses, would let the long loop run for minutes)")
    ap.add_argument("--max-iterations", type=int, default=30)
    ap.add_argument("--cases", default="tree+loops,one long loop")
    ap.add_argument("--json", default=None)
    ap.add_argument("--preconditioner", default="block_jacobi", choices=("block_jacobi", "tree"))
    ap.add_argument("--free-last", type=int, default=0, help="fix every pose but the last W before optimising (0: every pose is free)")
    ap.add_argument("--repeat", type=int, default=1, help="optimisations of a fresh copy of every graph; the fastest is reported (the counts are the same in each)")
    a = ap.parse_args()
    rows = []
    warm, _ = build(200, "tree+loops")
    warm.optimize(pcg_preconditioner=a.preconditioner)                     # code objects loaded, buffers of the runtime warm
    for n in [int(s) for s in a.sizes.split(",")]:
        for kind in a.cases.split(","):
            ms = None
            for _ in range(max(a.repeat, 1)):
                pg, n_loops = build(n, kind)
                if 0 < a.free_last < n:
                    pg.setFixed(0, n - a.free_last)
                t0 = time.perf_counter()
                out = pg.optimize(pcg_max_iterations=a.pcg_cap, max_iterations=a.max_iterations, pcg_preconditioner=a.preconditioner)
                t = (time.perf_counter() - t0) * 1e3
                ms = t if ms is None else min(ms, t)
            get_ms, set_ms, apply_ms = alternative_ms(pg, n)
            row = dict(poses=n, free=int(n - pg.fixed().sum()), case=kind, preconditioner=a.preconditioner, loops=n_loops, lm_iterations=out.iterations, accepted=out.accepted, pcg_iterations=out.pcg_iterations,
                       pcg_capped=out.pcg_capped, converged=out.converged, chi2_initial=out.chi2_initial, chi2_final=out.chi2_final, total_ms=ms,
                       us_per_pcg_iteration=1e3 * ms / max(out.pcg_iterations, 1), host_copy_out_ms=get_ms, set_poses_ms=set_ms, apply_to_ms=apply_ms)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
