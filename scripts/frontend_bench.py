"""The per-scan loop three ways over bench.py's extra.sequence drive (64 scans, 64 beams x 1024, its seed): sequence.drive over GpuFront (the loop in
Python), sequence.drive_frontend over pcr.Frontend (the loop in the library, called from Python) and lib/seq_harness (the loop in the library, called
from C++).  Per method: the first drive of a fresh session, then --passes drives after reset() on the same handles, the Python variants ALTERNATING so
that drift of the shared host hits them alike; the harness runs --harness-runs times with --reps 3.  Reported: scans/s (median, min, max over the
passes) and the host time of the five steps per scan.  profiles/frontend_notes.md holds a run.

    python scripts/frontend_bench.py [--scans 64] [--passes 15] [--out FILE.json] [--order python_loop,library_loop] [--baseline-sequence FILE]

One line per method goes to standard output; --out also writes everything as one JSON file.

--baseline-sequence: a copy of another revision's simpleslam_amd/sequence.py, whose drive(GpuFront) is timed in the same alternation ("parent")."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20261003      # bench.py's


def per_scan(ts, n):
    return {k: round(1e6 * v / n, 2) for k, v in ts.items()}


def spread(runs, n):
    sec = sorted(r["seconds"] for r in runs)
    med = sorted(runs, key=lambda r: r["seconds"])[len(runs) // 2]
    return dict(scans_per_s=dict(median=round(n / statistics.median(sec), 1), min=round(n / sec[-1], 1), max=round(n / sec[0], 1)),
                us_per_scan_median=round(1e6 * statistics.median(sec) / n, 2), step_us_per_scan=per_scan(med["step_seconds"], n), passes=len(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--harness-runs", type=int, default=3)
    ap.add_argument("--methods", default="loam,ndt,vgicp")
    ap.add_argument("--out", default=None)
    ap.add_argument("--order", default="python_loop,library_loop", help="the Python variants, in the order their registers are made and first driven")
    ap.add_argument("--baseline-sequence", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from simpleslam_amd import Frontend, make_register, sequence
    parent = None
    if args.baseline_sequence:
        spec = importlib.util.spec_from_file_location("simpleslam_amd.sequence_parent", args.baseline_sequence)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
    n = args.scans
    scans, truth, cmds = sequence.make_drive(n, SEED + 7)
    d_scans = [torch.from_numpy(s).cuda() for s in scans]
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "seq_harness")
    tmp = tempfile.mkdtemp(prefix="frontend_bench_")
    names = []
    for k, s in enumerate(scans):
        names.append(os.path.join(tmp, f"scan{k:03d}.f32"))
        np.ascontiguousarray(s, np.float32).tofile(names[-1])
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")
    open(os.path.join(tmp, "cmds.txt"), "w").write("".join(" ".join(repr(float(v)) for v in c.reshape(-1)) + "\n" for c in cmds))
    open(os.path.join(tmp, "start.txt"), "w").write(" ".join(repr(float(v)) for v in truth[0].reshape(-1)) + "\n")

    out = dict(workload=f"bench.py's extra.sequence drive: {n} scans, 64 beams x 1024, 0.5 m apart, grid 0.5 m, radius 8 m, key-frame gap 1 m; profile 0", methods={})
    for mth in args.methods.split(","):
        def fresh():
            reg = make_register(mth)
            reg.set_profile(0)
            return reg
        sequence.drive(sequence.GpuFront(fresh()), d_scans[:8], cmds[:8], truth[0])      # warm-up as bench.py's: code objects, first builds
        def make(name):      # -> (front or Frontend, callable running one drive)
            if name == "python_loop":
                fr = sequence.GpuFront(fresh())
                return fr, lambda pf=False: sequence.drive(fr, d_scans, cmds, truth[0], prefetch=pf)
            if name == "library_loop":
                fe = Frontend(fresh())
                return fe, lambda pf=False: sequence.drive_frontend(fe, d_scans, cmds, truth[0], prefetch=pf)
            if name == "parent_python_loop" and parent is not None:
                fp = parent.GpuFront(fresh())
                return fp, lambda pf=False: parent.drive(fp, d_scans, cmds, truth[0], prefetch=pf)
            raise SystemExit(f"--order: unknown variant {name} (parent_python_loop needs --baseline-sequence)")
        # the order matters: registers made one after the other in a process are not alike (profiles/frontend_notes.md) -- run every order you compare
        variants = {name: make(name) for name in args.order.split(",")}
        assert "python_loop" in variants, "--order must hold python_loop: its first drive is the reference of the pose comparison"
        res = {}
        firsts = {}
        for name, (obj, run) in variants.items():
            torch.cuda.synchronize()
            firsts[name] = run()
            res[name] = dict(first_drive=dict(scans_per_s=round(n / firsts[name]["seconds"], 1), step_us_per_scan=per_scan(firsts[name]["step_seconds"], n)))
        for pf in (False, True):
            runs = {name: [] for name in variants}
            for _ in range(args.passes):
                for name, (obj, run) in variants.items():      # alternating
                    obj.reset()
                    torch.cuda.synchronize()
                    runs[name].append(run(pf=pf))
            for name in variants:
                same = all(np.array_equal(a, b) for r in runs[name] for a, b in zip(r["poses"], firsts["python_loop"]["poses"]))
                res[name]["steady_prefetch" if pf else "steady"] = dict(spread(runs[name], n), poses_equal_python_first_drive=bool(same))
        # the C++ caller: its own process, its own handles; --reps 3: first drive and the third, after reset
        for pf in (False, True):
            hs = []
            for _ in range(args.harness_runs):
                t0 = time.perf_counter()
                p = subprocess.run([exe, mth, os.path.join(tmp, "list.txt"), os.path.join(tmp, "cmds.txt"), os.path.join(tmp, "start.txt"), "--reps", "3"] +
                                   (["--prefetch"] if pf else []), capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise RuntimeError(f"seq_harness {mth}: exit {p.returncode}: {p.stderr[-500:]}")
                rec = dict(process_seconds=round(time.perf_counter() - t0, 2))
                for ln in p.stdout.splitlines():
                    w = ln.split()
                    if w and w[0] == "summary":
                        kv = dict(zip(w[2::2], w[3::2]))
                        rec[w[1]] = dict(scans_per_s=float(kv["scans_per_s"]),
                                         step_us_per_scan={k: round(1e6 * float(kv[k]) / n, 2) for k in ("voxel", "wait", "scan2map", "add_keyframe", "update_map")})
                hs.append(rec)
            res["seq_harness_prefetch" if pf else "seq_harness"] = hs
        out["methods"][mth] = res
        print(mth, json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
        print("written", args.out)


if __name__ == "__main__":
    main()
