"""The shared cases of the deskew tests (tests/test_deskew_host.py, tests/test_deskew_gpu.py): small clouds with per-point times and a motion.

Point counts 1, 63, 64, 65 (a wave), 255, 256, 257 (the kernel's block of 256) and 4 099 (17 blocks, the last one partial); control poses K = 2, 3,
17 and 1 024; the three time kinds, packed (stride 16 and 20) and embedded (stride 32: a float or a u32 at byte 24 or 28, a double at byte 24);
t_ref at the start, at the end, inside and on either side of the range.  Every case of 63 points or more carries, in its first records, a time
exactly on the first stamp, on the last stamp and on an inner stamp (K >= 3), one before and one after the range, a NaN time (the float kinds), a
NaN coordinate and an infinite one.  Two motions start from rotations chosen for the quaternion rules: "flip" turns from Rz(-125 deg) to
Rz(-115 deg), whose extracted quaternions are (0, 0, +, -) and (0, 0, -, +) -- a negative dot product --, and "trace" passes a half turn about x,
where the trace is -1 and the quaternion comes from the largest diagonal element."""
import ctypes as C

import numpy as np

from deskew_ref import TIME_DTYPES, TIME_F32_SECONDS, TIME_F64_SECONDS, TIME_U32_NANOSECONDS


def _exp(xi):
    from simpleslam_amd import synth
    return synth.se3_exp(xi)


def rot_z(deg):
    return _exp([0, 0, 0, 0, 0, np.deg2rad(deg)])


def rot_x(deg):
    return _exp([0, 0, 0, np.deg2rad(deg), 0, 0])


def exact_stamps(base, kind, t0):
    """Stamps a time field of the kind can hit exactly: tau = t0 + field, formed as the library forms it -> (stamps, the fields that hit them)."""
    if kind == TIME_U32_NANOSECONDS:
        field = np.round(np.asarray(base) * 1e9).astype(np.uint32)
        return t0 + field.astype(np.float64) * 1e-9, field
    field = np.asarray(base).astype(TIME_DTYPES[kind])
    return t0 + field.astype(np.float64), field


def motion(K, seed, kind, t0=0.0, start=None, v=(2.0, 0.3, -0.1), w=(0.05, -0.08, 0.5), span=0.1, first=0.01):
    """K control poses of a constant twist (v m/s, w rad/s) from `start`, at jittered stamps in [first, first + span] -> (poses, stamps, fields)."""
    rng = np.random.default_rng([seed, 41])
    cuts = np.sort(rng.uniform(0.0, 1.0, K - 2)) if K > 2 else np.zeros(0)
    if K > 2:      # (jittered, but strictly increasing after the rounding to the time kind)
        cuts = (np.arange(1, K - 1) + 0.5 * (cuts - 0.5)) / (K - 1)
    base = first + span * np.concatenate([[0.0], cuts, [1.0]])
    stamps, fields = exact_stamps(base, kind, t0)
    assert (np.diff(stamps) > 0).all()
    start = np.eye(4) if start is None else start
    xi = np.concatenate([v, w])
    poses = np.stack([start @ _exp(xi * (s - stamps[0])) for s in stamps])
    return poses, stamps, fields


def make_case(name, n, K, kind, layout, t_ref_where, seed, inplace, t0=0.0, start=None, **motion_kw):
    """layout: ("packed", floats per record) or ("embedded", floats per record, byte offset of the time field)."""
    rng = np.random.default_rng([seed, 43])
    poses, stamps, fields = motion(K, seed, kind, t0, start, **motion_kw)
    lo, hi = stamps[0] - t0, stamps[-1] - t0
    cols = layout[1]
    cloud = rng.uniform(-60.0, 60.0, (n, cols)).astype(np.float32)
    dt = TIME_DTYPES[kind]
    if kind == TIME_U32_NANOSECONDS:
        t = np.round(rng.uniform(lo, hi, n) * 1e9).astype(np.uint32)
        before, after = np.uint32(0), np.uint32(round((hi + 0.05) * 1e9))
    else:
        t = rng.uniform(lo, hi, n).astype(dt)
        before, after = dt(lo - 0.02), dt(hi + 0.03)
    if n >= 63:
        t[0], t[1], t[3], t[4] = fields[0], fields[-1], before, after
        t[2] = fields[K // 2] if K >= 3 else fields[0]
        if kind != TIME_U32_NANOSECONDS:
            t[5] = np.nan
        cloud[6, 0] = np.nan
        cloud[7, 2] = np.inf
    times, offset = t, 0
    if layout[0] == "embedded":
        offset = layout[2]
        raw = cloud.view(np.uint8).reshape(n, cols * 4)
        raw[:, offset:offset + t.itemsize] = t.view(np.uint8).reshape(n, t.itemsize)
        times = None
    t_ref = {"start": stamps[0], "end": stamps[-1], "inside": 0.5 * (stamps[0] + stamps[-1]) + 1e-3, "before": stamps[0] - 1.0, "after": stamps[-1] + 1.0}[t_ref_where]
    return dict(name=name, cloud=cloud, times=times, kind=kind, offset=offset, poses=poses, stamps=stamps, t0=t0, t_ref=float(t_ref), inplace=inplace,
                expect_ref_clamped=int(t_ref_where in ("before", "after")))


def all_cases():
    F, U, D = TIME_F32_SECONDS, TIME_U32_NANOSECONDS, TIME_F64_SECONDS
    flip = rot_z(-125.0)                       # ten degrees on: Rz(-115), the other hemisphere of Eigen's extraction
    trace = rot_x(179.5) @ rot_z(20.0)         # half a degree on: the half turn about x
    return [
        make_case("n1_K2_f32_packed", 1, 2, F, ("packed", 4), "start", 1, False),
        make_case("n63_K3_u32_packed_inplace", 63, 3, U, ("packed", 4), "end", 2, True),
        make_case("n64_K17_f64_packed", 64, 17, D, ("packed", 4), "inside", 3, False),
        make_case("n65_K1024_f32_at24", 65, 1024, F, ("embedded", 8, 24), "after", 4, False),
        make_case("n255_K2_f32_at24_inplace", 255, 2, F, ("embedded", 8, 24), "before", 5, True),
        make_case("n256_K3_u32_at28", 256, 3, U, ("embedded", 8, 28), "inside", 6, False),
        make_case("n257_K17_f64_at24_inplace", 257, 17, D, ("embedded", 8, 24), "start", 7, True),
        make_case("n4099_K1024_f32_packed_epoch", 4099, 1024, F, ("packed", 4), "end", 8, False, t0=1700000000.0),
        make_case("n4099_K17_flip_stride20", 4099, 17, F, ("packed", 5), "inside", 9, True, start=flip, w=(0.0, 0.0, np.deg2rad(10.0) / 0.1 * 16), span=0.1),
        make_case("n257_K3_trace", 257, 3, D, ("packed", 4), "inside", 10, False, start=trace, w=(np.deg2rad(1.0) / 0.1, 0.0, 0.0)),
        make_case("n4099_K2_u32_packed", 4099, 2, U, ("packed", 4), "after", 11, False),
    ]


def negative_dot_somewhere(case):
    """Two consecutive control rotations whose extracted quaternions (before the sign rule) have a negative dot product."""
    from deskew_ref import quat_of
    q = [quat_of(T[:3, :3]) for T in case["poses"]]
    return any(float(a @ b) < 0 for a, b in zip(q, q[1:]))


def non_positive_trace_somewhere(case):
    return any(np.trace(T[:3, :3]) <= 0 for T in case["poses"])


# ---- the refusals, shared by the host and the GPU test ----

def raw_call(cloud, times, kind, offset, poses, stamps, t0, t_ref, out, K=None, stride=None, null=(), handle=None):
    """pcr_deskew_host -- or, with a register's handle, pcr_deskew on host memory -- through ctypes with nothing checked on the way -> (rc, message)."""
    from simpleslam_amd import load_library
    from simpleslam_amd.pcr import DeskewInfo, DeskewMotion
    L = load_library()
    dp = C.POINTER(C.c_double)
    cm = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(-1).copy()
    st = np.asarray(stamps, np.float64).copy()
    m = DeskewMotion(None if "poses" in null else cm.ctypes.data_as(dp), None if "stamps" in null else st.ctypes.data_as(dp),
                     len(st) if K is None else K, t0, t_ref)
    info = DeskewInfo()
    pts = None if "pts" in null else cloud.ctypes.data_as(C.c_void_p)
    tp = None if times is None else times.ctypes.data_as(C.c_void_p)
    mp = None if "m" in null else C.byref(m)
    op = None if "out" in null else out.ctypes.data_as(C.c_void_p)
    n, s = cloud.shape[0], cloud.shape[1] * 4 if stride is None else stride
    if handle is None:
        rc = L.pcr_deskew_host(pts, n, s, tp, kind, offset, mp, op, C.byref(info))
    else:
        rc = L.pcr_deskew(handle, pts, n, s, 0, tp, kind, offset, mp, op, 0, C.byref(info))
    return rc, L.pcr_last_error(handle).decode()


def refusals():
    """(name, the word the message must hold, keyword changes to a good call) -- shared with the GPU test."""
    nan, inf = float("nan"), float("inf")
    eye2 = np.tile(np.eye(4), (2, 1, 1))
    bad_pose = eye2.copy()
    bad_pose[1, 1, 2] = nan
    huge = eye2.copy()
    huge[0, 0, 0] = huge[0, 1, 1] = huge[0, 2, 2] = 1e308
    return [
        ("K_1", "K", dict(poses=eye2[:1], stamps=[0.0])),
        ("K_1025", "K", dict(poses=np.tile(np.eye(4), (1025, 1, 1)), stamps=np.arange(1025.0))),
        ("stamps_equal", "stamps", dict(stamps=[0.5, 0.5])),
        ("stamps_decreasing", "stamps", dict(stamps=[0.5, 0.25])),
        ("stamps_nan", "stamps", dict(stamps=[0.0, nan])),
        ("stamps_inf", "stamps", dict(stamps=[0.0, inf])),
        ("poses_nan", "poses", dict(poses=bad_pose)),
        ("poses_no_quaternion", "poses", dict(poses=huge)),
        ("t0_nan", "t0", dict(t0=nan)),
        ("t_ref_inf", "t_ref", dict(t_ref=inf)),
        ("time_kind_3", "time_kind", dict(kind=3)),
        ("time_kind_negative", "time_kind", dict(kind=-1)),
        ("offset_misaligned", "time_offset_bytes", dict(times=None, offset=18)),
        ("offset_past_the_stride", "time_offset_bytes", dict(times=None, offset=32)),
        ("offset_negative", "time_offset_bytes", dict(times=None, offset=-4)),
        ("offset_in_the_coordinates", "time_offset_bytes", dict(times=None, offset=8)),
        ("double_past_the_stride", "time_offset_bytes", dict(times=None, offset=24, kind=2, stride=28)),
        ("stride_12", "stride_bytes", dict(stride=12)),
        ("stride_odd", "stride_bytes", dict(stride=18)),
        ("pts_null", "pts", dict(null=("pts",))),
        ("out_null", "out", dict(null=("out",))),
        ("m_null", "m is NULL", dict(null=("m",))),
        ("poses_null", "poses", dict(null=("poses",))),
        ("stamps_null", "stamps", dict(null=("stamps",))),
    ]


def good_call():
    rng = np.random.default_rng(77)
    cloud = rng.uniform(-5, 5, (7, 8)).astype(np.float32)
    return dict(cloud=cloud, times=np.linspace(0.1, 0.9, 7).astype(np.float32), kind=0, offset=0, poses=np.tile(np.eye(4), (2, 1, 1)), stamps=[0.0, 1.0],
                t0=0.0, t_ref=0.0)
