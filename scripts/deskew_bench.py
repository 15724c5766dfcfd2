"""Measurements for profiles/deskew_notes.md, on one MI355X: the synchronous pcr_deskew call on a scan in HBM (65 536 points, K = 2 and 100), what a
caller pays on the host today (pcr_deskew_host plus the upload of its result), and extra.sequence's 64-scan drive through pcr_frontend_step against
pcr_frontend_step_timed with an identity motion (the same registration work: the difference is the deskew), on ONE front end, the two alternating
in both orders after a warm-up of each.  `python scripts/deskew_bench.py kernel` runs the device calls alone, for a kernel trace of its own
(rocprofv3 --kernel-trace -- python scripts/deskew_bench.py kernel).  Prints JSON."""
import sys, time, json
import numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import simpleslam_amd as sa
from simpleslam_amd import sequence, synth, make_register, Frontend, deskew, deskew_host
import deskew_cases, deskew_ref

out = {}
reg = make_register("loam")
n = 65536
rng = np.random.default_rng(1)
cloud = rng.uniform(-60, 60, (n, 4)).astype(np.float32)
times = np.sort(rng.uniform(0.0, 0.1, n)).astype(np.float32)
d_cloud, d_times, d_out = torch.from_numpy(cloud).cuda(), torch.from_numpy(times).cuda(), torch.empty((n, 4), dtype=torch.float32, device="cuda")
only = sys.argv[1] if len(sys.argv) > 1 else "all"
for K in (2, 100):
    poses, stamps, _ = deskew_cases.motion(K, 3, 0, first=0.0)
    for _ in range(50): deskew(reg, d_cloud, poses, stamps, times=d_times, t_ref=0.1, out=d_out)
    torch.cuda.synchronize()
    reps = 2000
    t = time.perf_counter()
    for _ in range(reps): deskew(reg, d_cloud, poses, stamps, times=d_times, t_ref=0.1, out=d_out)
    torch.cuda.synchronize()
    out[f"device_call_us_K{K}"] = (time.perf_counter() - t) / reps * 1e6
    if only == "kernel": continue
    reps = 50
    t = time.perf_counter()
    for _ in range(reps): h = deskew_host(cloud, poses, stamps, times=times, t_ref=0.1)[0]
    out[f"host_deskew_us_K{K}"] = (time.perf_counter() - t) / reps * 1e6
    t = time.perf_counter()
    for _ in range(reps):
        d = torch.from_numpy(h).cuda(); torch.cuda.synchronize()
    out[f"upload_us_K{K}"] = (time.perf_counter() - t) / reps * 1e6
    same = np.array_equal(d_out.cpu().numpy().view(np.uint32), h.view(np.uint32))
    out[f"device_equals_host_K{K}"] = bool(same)
print(json.dumps(out)); sys.stdout.flush()
if only == "kernel": sys.exit(0)

# the 64-scan drive: plain steps against timed steps with an identity motion (the registration's work is then the same: the difference is the deskew)
scans, truth, cmds = sequence.make_drive(64, 20261005)
d_scans = [torch.from_numpy(s).cuda() for s in scans]
d_t = torch.from_numpy((0.1 * (np.arange(scans[0].shape[0]) % 1024) / 1024).astype(np.float32)).cuda()
eye = np.tile(np.eye(4), (2, 1, 1))
def plain(fe):
    pose = np.array(truth[0], float); t = time.perf_counter()
    for k, s in enumerate(d_scans): pose, _ = fe.step(s, pose @ cmds[k])
    fe.finish(); return time.perf_counter() - t, pose
def timed(fe):
    pose = np.array(truth[0], float); t = time.perf_counter()
    for k, s in enumerate(d_scans): pose, _ = fe.stepTimed(s, pose @ cmds[k], eye, [0.0, 0.1], times=d_t, t_ref=0.1)
    fe.finish(); return time.perf_counter() - t, pose
for method in ("loam", "vgicp"):
    fe = Frontend(make_register(method))
    res = {"plain": [], "timed": []}
    last = {}
    for name, fn in (("plain", plain), ("timed", timed)):      # warm-up of both
        fn(fe); fe.reset()
    for order in (("plain", "timed"), ("timed", "plain"), ("plain", "timed"), ("timed", "plain")):
        for name in order:
            sec, pose = (plain if name == "plain" else timed)(fe); fe.reset()
            res[name].append(64 / sec); last[name] = pose
    out[f"drive_{method}_plain_scans_per_s"] = res["plain"]
    out[f"drive_{method}_timed_scans_per_s"] = res["timed"]
    out[f"drive_{method}_same_pose"] = bool(np.array_equal(last["plain"], last["timed"]))
    a, b = np.median(res["plain"]), np.median(res["timed"])
    out[f"drive_{method}_added_us_per_scan"] = (1 / b - 1 / a) * 1e6
print(json.dumps(out))
