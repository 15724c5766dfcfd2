"""Filling a ScanContext database from the key frames of one pcr_map (profiles/sc_add_keyframes_notes.md).

    python scripts/sc_add_keyframes_bench.py [--sizes 2000 20000] [--points 3000] [--grids 0 0.5] [--reps 5] [--lib PATH] [--json OUT]
For each N (key frames of --points random points each, 16-byte points, made on the device) and each grid_size, a FRESH database is filled
    per_frame: pcr_map_keyframe -> (pcr_voxel_filter, device to device, when grid_size > 0) -> pcr_sc_add, once per key frame: the only
               way before pcr_sc_add_keyframes (with --lib pointing at an older build this is all that is measured);
    batched:   one pcr_sc_add_keyframes over the range;
wall time from the first call to the return of the last one (every call ends synchronised), 1 warm-up and --reps repetitions each, median,
minimum and maximum reported.  The per-frame loop is driven through ctypes; `loop_overhead_ms` is what N x 3 trivial calls (pcr_sc_size)
cost from Python, to be read against per_frame.  The two databases' last descriptors are compared as a sanity check.  --large-points adds a
map of 200 key frames of that many points each, grid_size 0 only: the case in which a key frame is cut into slabs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fill_map(n_kf, points, seed):
    import torch
    from simpleslam_amd import SubMap
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    m = SubMap()
    T = np.eye(4)
    for _ in range(n_kf):
        r = torch.rand(points, generator=g, device="cuda") * 84.5 + 0.5
        a = (torch.rand(points, generator=g, device="cuda") * 2 - 1) * np.pi
        c = torch.stack([r * torch.cos(a), r * torch.sin(a), torch.rand(points, generator=g, device="cuda") * 12 - 2, torch.ones_like(r)], 1).contiguous()
        m.addKeyFrame(c, T)
    torch.cuda.synchronize()
    return m


def _stats(t):
    return dict(median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), runs_ms=[round(x, 3) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2000, 20000])
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--grids", type=float, nargs="+", default=[0.0, 0.5])      # 0.5: the reference's contextDownSampleGridSize
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large-points", type=int, default=0)
    ap.add_argument("--lib")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    from simpleslam_amd import pcr
    if a.lib:
        pcr.LIB_PATH = os.path.abspath(a.lib)
    from simpleslam_amd import LoamRegister, ScanContext
    L = pcr.load_library()
    batched = hasattr(L, "pcr_sc_add_keyframes")
    reg = LoamRegister()
    res = []

    def per_frame(sc, m, n_kf, grid, out):
        n, s, cnt = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        kf, vf, add, h, mm, ss, op = L.pcr_map_keyframe, L.pcr_voxel_filter, L.pcr_sc_add, reg._h, m._m, sc._s, C.c_void_p(out.data_ptr())
        for i in range(n_kf):
            p = kf(mm, i, C.byref(n), C.byref(s), None)
            if grid > 0 and n.value:
                if vf(h, p, n.value, s.value, 1, grid, op, n.value, 1, C.byref(cnt)):
                    raise RuntimeError(L.pcr_last_error(h).decode())
                p, n.value = op, cnt.value
            if add(ss, p, n.value, s.value, 1):
                raise RuntimeError(L.pcr_sc_last_error(ss).decode())

    def timed(fn, reps):
        t, last = [], None
        for r in range(reps + 1):
            sc = ScanContext()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(sc)
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                t.append(dt)
            last = sc
        return t, last

    cases = [(n, a.points, a.grids) for n in a.sizes] + ([(200, a.large_points, [0.0])] if a.large_points else [])
    for n_kf, points, grids in cases:
        m = _fill_map(n_kf, points, seed=n_kf)
        out = torch.empty((points, 4), dtype=torch.float32, device="cuda")
        probe, k = ScanContext(), C.c_size_t(0)
        t0 = time.perf_counter()
        for _ in range(3 * n_kf):
            L.pcr_sc_size(probe._s, C.byref(k))
        overhead = (time.perf_counter() - t0) * 1e3
        for grid in grids:
            row = dict(key_frames=n_kf, points_per_key_frame=points, grid_size=grid, loop_overhead_ms=round(overhead, 3))
            tp, sp = timed(lambda sc: per_frame(sc, m, n_kf, grid, out), a.reps if n_kf <= 2000 else min(a.reps, 3))
            row["per_frame"] = _stats(tp)
            if batched:
                tb, sb = timed(lambda sc: sc.addKeyFrames(m, 0, n_kf, grid), a.reps)
                row["batched"] = _stats(tb)
                row["ratio_per_frame_over_batched"] = round(row["per_frame"]["median_ms"] / row["batched"]["median_ms"], 2)
                row["same_last_descriptor"] = all(x.tobytes() == y.tobytes() for x, y in zip(sp.descriptor(n_kf - 1), sb.descriptor(n_kf - 1)))
                del sb
            del sp
            print(json.dumps(row), flush=True)
            res.append(row)
        del m
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
