"""Global relocalisation timings.

    python scripts/sc_rank_bench.py [--ranking-only] [--json OUT]
        1. pcr_sc_distances against databases of M = 1 000, 10 000, 100 000 contexts (filled by pcr_sc_add from cheap random clouds):
           median wall time, descriptor bytes per second (4 800 B x M), and the host loop of pcr_sc_distance over the same contexts;
        2. (not with --ranking-only) pcr_relocalize_global, LOAM, on a 1 M-point map with ~500 key frames: median wall time and its split
           into ranking, the batched coarse score and the refinements, each timed on its own with the same inputs.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sc -- python scripts/sc_rank_bench.py --ranking-only
    python scripts/sc_rank_bench.py --summarise DIR OUT.csv
        kernel-only durations of sc_rank_kernel (one row per grid size, i.e. per M) and sc_query_keys_kernel from the trace."""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("sc_rank_kernel", "sc_query_keys_kernel", "sc_polar_kernel")


def summarise(d, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = {}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
                if name is None:
                    continue
                grid = int(r.get("Grid_Size") or r.get("Grid_Size_X"))
                dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
                rows.setdefault((name, grid), []).append(dur)
    table = [("kernel", "grid_threads", "dispatches", "median_us", "total_us")]
    for (name, grid), v in sorted(rows.items()):
        if name == "sc_polar_kernel" and len(v) > 1000:
            continue      # (the database fills: one binning per context)
        table.append((name, grid, len(v), round(float(np.median(v)), 3), round(float(np.sum(v)), 1)))
    with open(out, "w", newline="") as fh:
        csv.writer(fh).writerows(table)
    for r in table:
        print(*r, sep=",")


def _median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def ranking(res):
    from simpleslam_amd import ScanContext
    rng = np.random.default_rng(1)
    q = np.zeros((20000, 4), np.float32)
    r = rng.uniform(1.0, 85.0, len(q)); a = rng.uniform(-np.pi, np.pi, len(q))
    q[:, 0], q[:, 1], q[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 10.0, len(q))
    sc = ScanContext()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for M in (1_000, 10_000, 100_000):
        while len(sc) < M:
            c = np.zeros((300, 4), np.float32)
            r = rng.uniform(1.0, 85.0, 300); a = rng.uniform(-np.pi, np.pi, 300)
            c[:, 0], c[:, 1], c[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 10.0, 300)
            sc.addContext(c)
        sc.distances(q)
        dev_ms = _median_ms(lambda: sc.distances(q), 30)
        dist, shift = sc.distances(q)
        # the host loop: the query added as context M, compared with contexts 0 .. M-1
        sc.addContext(q)
        d, s = C.c_double(0), C.c_int(0)
        L, h = sc._lib, sc._s
        t0 = time.perf_counter()
        same = True
        for i in range(M):
            L.pcr_sc_distance(h, M, i, C.byref(d), C.byref(s))
            same = same and d.value == dist[i] and s.value == shift[i]
        host_ms = (time.perf_counter() - t0) * 1e3
        row = dict(M=M, device_ms=round(dev_ms, 3), descriptor_GBps=round(4800 * M / (dev_ms * 1e-3) / 1e9, 1), host_loop_ms=round(host_ms, 1),
                   speedup=round(host_ms / dev_ms, 1), equal_to_host=bool(same))
        print(json.dumps(row), flush=True)
        res.setdefault("ranking", []).append(row)
        # (the database now holds M + 1 contexts; the next size fills up from there)


def whole_call(res):
    from simpleslam_amd import LoamRegister, ScanContext, global_reloc_hypotheses, global_reloc_params, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import global_reloc_scene
    # 7 x 7 blocks; eight buildings dropped where no quarter turn of the square maps one onto another (the plain grid repeats every place)
    world, m = global_reloc_scene.asymmetric_world(1_000_000, seed=3, dropped=((1, 0), (1, 6), (2, 0), (2, 3), (3, 0), (4, 1), (5, 2), (6, 0)))
    mid = (world.blocks // 2) * synth.PITCH

    def planar(x, y, yaw):
        T = np.eye(4)
        T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
        T[:3, 3] = np.array([x, y, synth.SENSOR_Z]) - synth.map_origin(world.blocks)
        return T

    kf = [planar(x, y, 0.0) for y in (mid - 50.0, mid, mid + 50.0) for x in np.arange(20.0, world.side - 20.0, 2.0)]
    kf = np.array(kf[:500])
    sc = ScanContext()
    t0 = time.perf_counter()
    for i, T in enumerate(kf):
        sc.addContext(synth.make_scan(world, 0, seed=900 + i, beams=32, azimuths=720, pose=T)[0])
    print(f"{len(kf)} key frames in {time.perf_counter() - t0:.1f} s", flush=True)
    truth = planar(126.7, mid + 0.6, math.radians(131.0))      # next to the dropped building (2, 3)
    scan = synth.make_scan(world, 0, seed=5, beams=32, azimuths=720, pose=truth)[0]      # 23 040 points, as the key frames
    reg = LoamRegister()
    reg.setTarget(m)
    pose = np.eye(4)
    reg.relocalizeGlobal(scan, sc, kf, pose)
    total = _median_ms(lambda: reg.relocalizeGlobal(scan, sc, kf, np.eye(4)), 5)
    _, cands, chosen = reg.relocalizeGlobal(scan, sc, kf, pose)
    rank_ms = _median_ms(lambda: sc.distances(scan), 10)
    p = global_reloc_params()
    dist, shift = sc.distances(scan)
    places = np.lexsort((np.arange(len(dist)), dist))[:p.places]
    lattice = np.concatenate([global_reloc_hypotheses(kf[i], int(shift[i])) for i in places])
    coarse_ms = _median_ms(lambda: reg.fitnessBatch(scan, lattice, 1.0, 4096), 5)
    starts = [global_reloc_hypotheses(kf[c["place"]], c["sc_shift"])[c["hypothesis"]] for c in cands]

    def refine():
        for s in starts:
            reg.align(scan, s.copy())
    refine_ms = _median_ms(refine, 3)
    final_ms = _median_ms(lambda: reg.fitnessBatch(scan, np.array([c["pose"] for c in cands]), 1.0, 0), 5)
    et, er = synth.pose_error(pose, truth)
    row = dict(map_points=len(m), top_place_m=round(float(np.linalg.norm(kf[places[0]][:2, 3] - truth[:2, 3])), 2), key_frames=len(kf), scan_points=len(scan), hypotheses=len(lattice), candidates=len(cands), total_ms=round(total, 2),
               ranking_ms=round(rank_ms, 3), coarse_ms=round(coarse_ms, 3), refine_ms=round(refine_ms, 2), final_score_ms=round(final_ms, 3),
               error_m=round(et, 4), error_deg=round(math.degrees(er), 3))
    print(json.dumps(row), flush=True)
    res["whole_call"] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranking-only", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--summarise", nargs=2, metavar=("DIR", "OUT"))
    a = ap.parse_args()
    if a.summarise:
        summarise(*a.summarise)
        return
    res = {}
    ranking(res)
    if not a.ranking_only:
        whole_call(res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
