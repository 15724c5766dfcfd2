"""pcr_voxel_filter_sparse (V3 and V2) next to pcr_voxel_filter, device-resident in and out: medians after warm-up on a 65 536-point scan, a
1 M-point map and a 10 M-point map at 0.4 m; then the two clouds of DESIGN 4.5 whose dense table took tens of GB -- the 1290^3 cube at 0.1 m
and the flat cloud 2 km across at 0.05 m -- with the time and the device memory the handle holds.
    python scripts/quick_voxel_sparse.py [--only scan|map1m|map10m|cube|flat] [--reps 20]
(pcr_voxel_filter's code is the parent commit's, unchanged: its column is the parent's figure measured in the same process.)"""
import argparse
import gc
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import torch
from simpleslam_amd import LoamRegister, synth

ap = argparse.ArgumentParser()
ap.add_argument('--only', default='')
ap.add_argument('--reps', type=int, default=20)
args = ap.parse_args()
S = 20261003 + 2


def median_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def held(f):
    """f on a handle of its own -> (result, device memory the handle holds afterwards, bytes)"""
    torch.cuda.synchronize(); gc.collect()
    free0, _ = torch.cuda.mem_get_info()
    reg = LoamRegister()
    out = f(reg)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    reg.close()
    return out, free0 - free1


w, m = synth.make_map(1_000_000, seed=S)
scan, T = synth.make_scan(w, 0, seed=S)
cases = [('scan', 'scan 65536', scan), ('map1m', 'map 1M', m)]
if args.only in ('', 'map10m'):
    big = np.concatenate([m + np.array([400.0 * (k % 5), 400.0 * (k // 5), 0, 0], np.float32) for k in range(10)])
    cases.append(('map10m', 'map 10M', big))
for key, name, pts in cases:
    if args.only and args.only != key:
        continue
    d = torch.from_numpy(pts).cuda()
    reg = LoamRegister()
    reps = args.reps if len(pts) < 5_000_000 else max(args.reps // 4, 3)
    pcl, pcl_min = median_ms(lambda: reg.voxelDownSample(d, 0.4), reps)
    n_pcl = reg.voxelDownSample(d, 0.4).shape[0]
    v3, v3_min = median_ms(lambda: reg.voxelDownSampleV3(d, 0.4), reps)
    n3 = reg.voxelDownSampleV3(d, 0.4).shape[0]
    v2, v2_min = median_ms(lambda: reg.voxelDownSampleV2(d, 0.4), reps)
    n2 = reg.voxelDownSampleV2(d, 0.4).shape[0]
    print(f'{name} leaf 0.4: {len(pts)} rows | pcr_voxel_filter {pcl:.3f} ms (min {pcl_min:.3f}) -> {n_pcl} | V3 {v3:.3f} ms (min {v3_min:.3f}) -> {n3}, x{v3 / pcl:.2f} | '
          f'V2 {v2:.3f} ms (min {v2_min:.3f}) -> {n2}, x{v2 / pcl:.2f}', flush=True)
    reg.close(); del d, reg

rng = np.random.default_rng(8)
if args.only in ('', 'cube'):      # tests/test_voxel_edges_gpu.py: test_the_1290_cube_just_under_the_limit_is_filtered, with a million points inside
    pts = np.zeros((1_000_000, 4), np.float32)
    pts[:, :3] = rng.random((1_000_000, 3)) * 128.9
    pts[0, :3] = [0.05, 0.0, 0.0]; pts[1, :3] = [129.0, 128.95, 128.95]
    d = torch.from_numpy(pts).cuda()
    warm = torch.empty_like(d); del warm      # (the output's block is in torch's cache before the handle's memory is measured)
    for kind in ('voxelDownSampleV3', 'voxelDownSampleV2'):
        (ms, n_out), mem = held(lambda r: (median_ms(lambda: getattr(r, kind)(d, 0.1), 5)[0], getattr(r, kind)(d, 0.1).shape[0]))
        print(f'1290^3 cube, 1 M rows, leaf 0.1, {kind}: {ms:.3f} ms -> {n_out} voxels, handle holds {mem / 1e6:.1f} MB (dense table: 54.5 GB)', flush=True)
if args.only in ('', 'flat'):
    n = 1_000_000
    pts = np.zeros((n, 4), np.float32)
    pts[:, :2] = rng.random((n, 2)) * 2000.0 - 1000.0
    pts[:4, :2] = [[-1000, -1000], [1000, 1000], [-1000, 1000], [1000, -1000]]
    pts[:, 2] = 0.02
    d = torch.from_numpy(pts).cuda()
    warm = torch.empty_like(d); del warm      # (the output's block is in torch's cache before the handle's memory is measured)
    for kind in ('voxelDownSampleV3', 'voxelDownSampleV2'):
        (ms, n_out), mem = held(lambda r: (median_ms(lambda: getattr(r, kind)(d, 0.05), 5)[0], getattr(r, kind)(d, 0.05).shape[0]))
        print(f'flat 2 km, 1 M rows, leaf 0.05, {kind}: {ms:.3f} ms -> {n_out} voxels, handle holds {mem / 1e6:.1f} MB (dense table: 38.4 GB)', flush=True)
