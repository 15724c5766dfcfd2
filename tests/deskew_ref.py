"""pcr_deskew's definition (include/pcr_hip.h, csrc/deskew_math.h) restated in numpy: every operation an IEEE double operation of its own, in the
association the header fixes, so the result equals pcr_deskew_host's bit for bit.  No library call."""
import numpy as np

TIME_F32_SECONDS, TIME_U32_NANOSECONDS, TIME_F64_SECONDS = 0, 1, 2
TIME_DTYPES = {TIME_F32_SECONDS: np.float32, TIME_U32_NANOSECONDS: np.uint32, TIME_F64_SECONDS: np.float64}


def quat_of(R):
    """Eigen's Quaternion(Matrix3) as small_math.h's t2se3 has it, normalised -> (x, y, z, w)."""
    R = np.asarray(R, np.float64)
    q = np.zeros(4)
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(((R[i, i] - R[j, j]) - R[k, k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def table(poses, stamps):
    """(K, 8): the quaternion with the sign rule, the translation, the stamp."""
    poses = np.asarray(poses, np.float64)
    tab = np.zeros((poses.shape[0], 8))
    for j, T in enumerate(poses):
        q = quat_of(T[:3, :3])
        if j:
            p = tab[j - 1, :4]
            if ((q[0] * p[0] + q[1] * p[1]) + q[2] * p[2]) + q[3] * p[3] < 0.0:
                q = -q
        tab[j, :4] = q
        tab[j, 4:7] = T[:3, 3]
        tab[j, 7] = stamps[j]
    return tab


def evaluate(tab, tau):
    """The trajectory at times tau (m,) -> (R (m, 3, 3), p (m, 3), clamped (m,) in {-1, 0, +1}), vectorised."""
    tau = np.asarray(tau, np.float64).reshape(-1)
    st = tab[:, 7]
    K = tab.shape[0]
    clamped = np.where(tau < st[0], -1, np.where(tau > st[-1], 1, 0))
    tc = np.where(tau < st[0], st[0], np.where(tau > st[-1], st[-1], tau))
    j = np.clip(np.searchsorted(st, tc, side="right") - 1, 0, K - 2)      # the largest j of [0, K - 2] with st[j] <= tau
    a, b = tab[j], tab[j + 1]
    s = (tc - a[:, 7]) / (b[:, 7] - a[:, 7])
    u = 1.0 - s
    v = u[:, None] * a[:, :7] + s[:, None] * b[:, :7]
    q, p = v[:, :4], v[:, 4:7]
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    x, y, z, w = q[:, 0] / n, q[:, 1] / n, q[:, 2] / n, q[:, 3] / n
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.empty((tau.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R, p, clamped


def point_times(cloud, times, time_kind, time_offset, t0):
    """tau of every record, in double."""
    if times is None:
        raw = np.ascontiguousarray(cloud).view(np.uint8).reshape(cloud.shape[0], -1)
        width = np.dtype(TIME_DTYPES[time_kind]).itemsize
        field = np.ascontiguousarray(raw[:, time_offset:time_offset + width]).view(TIME_DTYPES[time_kind]).reshape(-1)
    else:
        field = np.asarray(times, TIME_DTYPES[time_kind]).reshape(-1)
    if time_kind == TIME_U32_NANOSECONDS:
        return t0 + field.astype(np.float64) * 1e-9
    with np.errstate(invalid="ignore"):
        return t0 + field.astype(np.float64)


def deskew(cloud, poses, stamps, times=None, time_kind=TIME_F32_SECONDS, time_offset=0, t0=0.0, t_ref=0.0):
    """-> (out float32 of the cloud's shape, info dict)"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    tab = table(poses, stamps)
    with np.errstate(invalid="ignore"):
        tau = point_times(cloud, times, time_kind, time_offset, float(t0))
        xyz = cloud[:, :3].astype(np.float64)
        ok = np.isfinite(xyz).all(1) & np.isfinite(tau)
    Rr, pr, cr = evaluate(tab, [t_ref])
    Rr, pr = Rr[0], pr[0]
    out = cloud.copy()
    x = xyz[ok]
    R, p, cl = evaluate(tab, tau[ok])
    d = [(((R[:, r, 0] * x[:, 0] + R[:, r, 1] * x[:, 1]) + R[:, r, 2] * x[:, 2]) + p[:, r]) - pr[r] for r in range(3)]
    z = np.stack([(Rr[0, c] * d[0] + Rr[1, c] * d[1]) + Rr[2, c] * d[2] for c in range(3)], 1)
    out[ok, :3] = z.astype(np.float32)
    return out, dict(before=int((cl < 0).sum()), after=int((cl > 0).sum()), nonfinite=int((~ok).sum()), ref_clamped=int(cr[0] != 0))
