"""The liorf method restated in numpy float32: LioScan2map of the reference's test/comp/liorf_scan2map.cpp, as DESIGN.md ("liorf") defines it.

Every float operation of the per-point stage is written on its own, in the kernel's order (the library is built without FMA contraction and
+ - * / sqrt are IEEE on both sides), so a float32 numpy array goes through the same roundings as a lane of the kernel.  The 21 + 6 sums are
taken exactly (math.fsum of products formed in float64, which are exact) and rounded to float once; the 6 x 6 solve is the same unpivoted
Householder QR in float32.  sinf / cosf / atan2f / asinf are the C library's, through ctypes.

Also here: the margins of a linearisation to the method's gates and the condition numbers of its patches (the inputs are tests/liorf_cases.py's).
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

F = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "asinf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]
_libm.atan2f.restype = C.c_float
_libm.atan2f.argtypes = [C.c_float, C.c_float]

DEFAULTS = dict(iters=30, knn_max_sq=1.0, plane_thresh=0.2, point_thresh=0.1, min_rows=50, min_scan=30, rot_conv_deg=0.05, trans_conv_cm=0.05,
                degenerate_eig=100.0, file_row=False)


def sinf(x):
    return F(_libm.sinf(float(F(x))))


def cosf(x):
    return F(_libm.cosf(float(F(x))))


# ---- the two PCL functions ----------------------------------------------------------------------------------------------------------
def pose_to_6dof(T):
    """pcl::getEulerAngles + the translation, of the float cast of a 4x4 pose: [roll, pitch, yaw, x, y, z] float32"""
    t = np.asarray(T, np.float64).astype(F)
    return np.array([_libm.atan2f(float(t[2, 1]), float(t[2, 2])), _libm.asinf(float(-t[2, 0])), _libm.atan2f(float(t[1, 0]), float(t[0, 0])),
                     t[0, 3], t[1, 3], t[2, 3]], F)


def transformation(six, trig=None):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) in float32: (4, 4)"""
    six = np.asarray(six, F)
    if trig is None:
        trig = (cosf(six[2]), sinf(six[2]), cosf(six[1]), sinf(six[1]), cosf(six[0]), sinf(six[0]))
    A, B, Cc, D, E, Fs = (F(v) for v in trig)
    T = np.zeros((4, 4), F)
    T[0] = [A * Cc, A * D * Fs - B * E, B * Fs + A * D * E, six[3]]
    T[1] = [B * Cc, A * E + B * D * Fs, B * D * E - A * Fs, six[4]]
    T[2] = [-D, Cc * Fs, Cc * E, six[5]]
    T[3, 3] = 1
    return T


# ---- the search: PCL's float metric, ties on the lower index --------------------------------------------------------------------------
def knn_f32(tgt, q, k, chunk=128):
    """-> (idx (n, k) int64, d2 (n, k) float32): d = dx dx; d += dy dy; d += dz dz in float32, ascending by (d, row).  Target rows that are
    not finite are left out and do not renumber the others."""
    P = np.asarray(tgt, F)[:, :3]
    rows = np.flatnonzero(np.isfinite(P).all(axis=1))
    P = P[rows]
    q = np.asarray(q, F)
    n = q.shape[0]
    idx = np.full((n, k), -1, np.int64)
    d2 = np.full((n, k), np.inf, F)
    m = min(k, len(rows))
    for s in range(0, n, chunk):
        c = q[s:s + chunk]
        dx = c[:, None, 0] - P[None, :, 0]
        d = dx * dx
        dy = c[:, None, 1] - P[None, :, 1]
        d += dy * dy
        dz = c[:, None, 2] - P[None, :, 2]
        d += dz * dz
        kk = min(m + 3, d.shape[1])
        part = np.argpartition(d, kk - 1, axis=1)[:, :kk] if kk < d.shape[1] else np.tile(np.arange(d.shape[1]), (d.shape[0], 1))
        # every row at a distance <= the kk-th smallest, so that ties at the edge are all there; then (d, row) order
        for j in range(d.shape[0]):
            thr = d[j, part[j]].max()
            cand = np.flatnonzero(d[j] <= thr)
            o = np.lexsort((cand, d[j, cand]))[:m]
            idx[s + j, :m] = rows[cand[o]]
            d2[s + j, :m] = d[j, cand[o]]
    return idx, d2


# ---- the plane fit: Eigen::ColPivHouseholderQR<Matrix<float,5,3>>::solve(-1), one patch at a time ---------------------------------------
def plane_qr_solve(a):
    a = np.array(a, F)
    c = np.full(5, -1, F)
    perm = [0, 1, 2]
    tau = np.zeros(3, F)
    nu = np.zeros(3, F)
    maxn = F(0)
    for j in range(3):
        s = F(0)
        for i in range(5):
            s = s + a[i, j] * a[i, j]
        nu[j] = np.sqrt(s)
        if nu[j] > maxn:
            maxn = nu[j]
    nd = nu.copy()
    eps = F(1.1920928955078125e-07)
    thr_helper = (maxn * eps) * (maxn * eps) / F(5)
    downdate_thr = F(3.4526698300124393e-04)
    nonzero = 3
    with np.errstate(all="ignore"):
        for k in range(3):
            big, bign = k, nu[k]
            for j in range(k + 1, 3):
                if nu[j] > bign:
                    bign, big = nu[j], j
            if nonzero == 3 and bign * bign < thr_helper * F(5 - k):
                nonzero = k
            if big != k:
                a[:, [k, big]] = a[:, [big, k]]
                nu[[k, big]] = nu[[big, k]]
                nd[[k, big]] = nd[[big, k]]
                perm[k], perm[big] = perm[big], perm[k]
            tail_sq = F(0)
            for i in range(k + 1, 5):
                tail_sq = tail_sq + a[i, k] * a[i, k]
            c0 = a[k, k]
            tiny = tail_sq <= F(1.1754943508222875e-38)
            beta = np.sqrt(c0 * c0 + tail_sq)
            beta = -beta if c0 >= 0 else beta
            den = c0 - beta
            for i in range(k + 1, 5):
                a[i, k] = F(0) if tiny else a[i, k] / den
            tau[k] = F(0) if tiny else (beta - c0) / beta
            a[k, k] = c0 if tiny else beta
            for j in range(k + 1, 3):
                tmp = F(0)
                for i in range(k + 1, 5):
                    tmp = tmp + a[i, k] * a[i, j]
                tmp = tmp + a[k, j]
                a[k, j] = a[k, j] - tau[k] * tmp
                for i in range(k + 1, 5):
                    a[i, j] = a[i, j] - tau[k] * a[i, k] * tmp
            for j in range(k + 1, 3):
                nz = nu[j] != 0
                temp = np.abs(a[k, j]) / nu[j]
                temp = (F(1) + temp) * (F(1) - temp)
                temp = F(0) if temp < 0 else temp
                r = nu[j] / nd[j]
                recompute = temp * r * r <= downdate_thr
                s = F(0)
                for i in range(k + 1, 5):
                    s = s + a[i, j] * a[i, j]
                root = np.sqrt(s if recompute else temp)
                nu_new = root if recompute else nu[j] * root
                if nz and recompute:
                    nd[j] = root
                if nz:
                    nu[j] = nu_new
        for k in range(min(nonzero, 3)):
            tmp = F(0)
            for i in range(k + 1, 5):
                tmp = tmp + a[i, k] * c[i]
            tmp = tmp + c[k]
            c[k] = c[k] - tau[k] * tmp
            for i in range(k + 1, 5):
                c[i] = c[i] - tau[k] * a[i, k] * tmp
        y = np.zeros(3, F)
        for i in range(2, -1, -1):
            if i >= nonzero:
                continue
            s = c[i]
            for j in range(i + 1, 3):
                if j < nonzero:
                    s = s - a[i, j] * y[j]
            y[i] = s / a[i, i]
    x = np.zeros(3, F)
    for i in range(3):
        x[perm[i]] = y[i] if i < nonzero else F(0)
    return x


# ---- surfOptimization + the rows of LMOptimization --------------------------------------------------------------------------------------
def per_point(scan, tgt, T, sc=None, prm=DEFAULTS):
    """The per-point stage at the float 4x4 T.  -> dict(kept (n,) bool, coeff (n, 4) float32, rows (n, 6) float32 (with sc), d2 (n, 6) float32 =
    the six nearest squared distances, resid (n,) = the largest plane residual, s (n,) float32; NaN where a stage was not reached)."""
    P = np.asarray(scan, F)[:, :3]
    tg = np.asarray(tgt, F)[:, :3]
    T = np.asarray(T, F)
    n = P.shape[0]
    kept = np.zeros(n, bool)
    coeff = np.zeros((n, 4), F)
    rows = np.zeros((n, 6), F)
    resid = np.full(n, np.nan)
    sval = np.full(n, np.nan, F)
    fin = np.isfinite(P).all(axis=1)
    with np.errstate(all="ignore"):
        q = np.stack([T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1] + T[r, 2] * P[:, 2] + T[r, 3] for r in range(3)], axis=1)
    d2 = np.full((n, 6), np.inf, F)
    idx = np.full((n, 6), -1, np.int64)
    if fin.any():
        idx[fin], d2[fin] = knn_f32(tg, q[fin], 6)
    thr_knn, thr_plane, thr_point = float(prm["knn_max_sq"]), float(prm["plane_thresh"]), float(prm["point_thresh"])
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(fin):
            if not (idx[i, 4] >= 0 and float(d2[i, 4]) < thr_knn):
                continue
            nb = tg[idx[i, :5]]
            X = plane_qr_solve(nb)
            pa, pb, pc, pd = X[0], X[1], X[2], F(1)
            ps = np.sqrt(pa * pa + pb * pb + pc * pc)
            pa, pb, pc, pd = pa / ps, pb / ps, pc / ps, pd / ps
            res = np.abs(pa * nb[:, 0] + pb * nb[:, 1] + pc * nb[:, 2] + pd)
            resid[i] = float(res.max()) if np.isfinite(res).all() else np.nan
            if (res.astype(np.float64) > thr_plane).any():
                continue
            pd2 = pa * q[i, 0] + pb * q[i, 1] + pc * q[i, 2] + pd
            den = np.sqrt(np.sqrt(P[i, 0] * P[i, 0] + P[i, 1] * P[i, 1] + P[i, 2] * P[i, 2]))
            s = F(1.0 - 0.9 * float(np.abs(pd2)) / float(den))
            sval[i] = s
            if not float(s) > thr_point:
                continue
            kept[i] = True
            coeff[i] = [s * pa, s * pb, s * pc, s * pd2]
    if sc is not None:
        cx, cy, cz = coeff[:, 0], coeff[:, 1], coeff[:, 2]
        with np.errstate(all="ignore"):
            arz, ary, arx = angular_entries(np.asarray(sc, F), P[:, 0], P[:, 1], P[:, 2], cx, cy, cz)
        rows = np.stack([arz, ary, arx, cx, cy, cz], axis=1).astype(F)
        rows[~kept] = 0
    return dict(kept=kept, coeff=coeff, rows=rows, d2=d2, idx=idx, resid=resid, s=sval, q=q)


def row_matrices(sr, cr, sp, cp, sy, cy, file_row=False):
    """The three 3 x 3 matrices behind the angular entries of a row, stacked (3, 3, 3) for roll, pitch, yaw: the derivative of
    Rz(yaw) Ry(pitch) Rx(roll) with respect to each angle.  liorf_scan2map.cpp:306-315 writes out the same matrices except for the pitch
    matrix's entry (1, 1), where its line 310 has sin(pitch) in place of the derivative's cos(pitch); the method takes the derivative
    ("liorf").  In the type of the arguments, every product left to right."""
    z = sr * 0
    Gr = [[z, cy * sp * cr + sy * sr, sy * cr - cy * sp * sr], [z, sy * sp * cr - cy * sr, -(sy * sp * sr) - cy * cr], [z, cp * cr, -(cp * sr)]]
    Gp = [[-(cy * sp), cy * cp * sr, cy * cp * cr], [-(sy * sp), sy * (sp if file_row else cp) * sr, sy * cp * cr], [-cp, -(sp * sr), -(sp * cr)]]
    Gy = [[-(sy * cp), -(sy * sp * sr + cy * cr), cy * sr - sy * sp * cr], [cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [z, z, z]]
    return np.array([Gr, Gp, Gy], dtype=np.asarray(sr).dtype)


def angular_entries(G, px, py, pz, cx, cy, cz):
    """coeff . (G_a p) for a = roll, pitch, yaw: the first three entries of a row, every sum left to right"""
    out = []
    for g in G:
        u = [g[r, 0] * px + g[r, 1] * py + g[r, 2] * pz for r in range(3)]
        out.append(u[0] * cx + u[1] * cy + u[2] * cz)
    return out


def row_trig(six, file_row=False):
    """The rows' matrices at the six numbers, float32, from the C library's sinf / cosf (file_row: pcr_params.liorf_file_row)"""
    six = np.asarray(six, F)
    return row_matrices(sinf(six[0]), cosf(six[0]), sinf(six[1]), cosf(six[1]), sinf(six[2]), cosf(six[2]), file_row)


def sums(rows, coeff, kept):
    """AtA (6, 6), AtB (6,) in float64: exact sums of the exact products, rounded once"""
    R = rows[kept].astype(np.float64)
    b = -coeff[kept, 3].astype(np.float64)
    AtA = np.zeros((6, 6))
    AtB = np.zeros(6)
    for r in range(6):
        for c in range(r, 6):
            AtA[r, c] = AtA[c, r] = math.fsum(R[:, r] * R[:, c])
        AtB[r] = math.fsum(R[:, r] * b)
    return AtA, AtB


def qr6_solve(A, b):
    """A x = b by unpivoted Householder QR in float32 ("liorf")"""
    a = np.array(A, F)
    b = np.array(b, F)
    with np.errstate(all="ignore"):
        for k in range(6):
            nrm2 = F(0)
            for i in range(k, 6):
                nrm2 = nrm2 + a[i, k] * a[i, k]
            nrm = np.sqrt(nrm2)
            alpha = -nrm if a[k, k] > 0 else nrm
            v = a[:, k].copy()
            v[k] = v[k] - alpha
            vv = F(0)
            for i in range(k, 6):
                vv = vv + v[i] * v[i]
            if not vv > 0:
                continue
            for j in list(range(k + 1, 6)) + [None]:
                col = b if j is None else a[:, j]
                dot = F(0)
                for i in range(k, 6):
                    dot = dot + v[i] * col[i]
                f = F(2) * dot / vv
                for i in range(k, 6):
                    col[i] = col[i] - f * v[i]
            a[k, k] = alpha
        x = np.zeros(6, F)
        for i in range(5, -1, -1):
            s = b[i]
            for j in range(i + 1, 6):
                s = s - a[i, j] * x[j]
            x[i] = s / a[i, i] if a[i, i] != 0 else F(0)
    return x


def scan2map(scan, tgt, T0, prm=DEFAULTS):
    """scan2MapOptimization from the 4x4 guess T0.  -> dict(pose (4, 4) float64 of float values, six, converged, iterations, degenerate,
    rows_last, min_eig (numpy eigvalsh of iteration 0's float system, or None), last_deltas (deltaR, deltaT of the last solved step))"""
    six = pose_to_6dof(T0)
    n = np.asarray(scan).shape[0]
    out = dict(converged=False, iterations=0, degenerate=False, rows_last=0, min_eig=None, last_deltas=None)
    if n > prm["min_scan"]:
        for it in range(prm["iters"]):
            pp = per_point(scan, tgt, transformation(six), row_trig(six, prm.get("file_row", False)), prm)
            out["iterations"] += 1
            out["rows_last"] = int(pp["kept"].sum())
            if out["rows_last"] < prm["min_rows"]:
                break      # the file's loop repeats this linearisation unchanged until its cap: the method stops here
            AtA, AtB = sums(pp["rows"], pp["coeff"], pp["kept"])
            A32, b32 = AtA.astype(F), AtB.astype(F)
            x = qr6_solve(A32, b32)
            if it == 0:
                out["min_eig"] = float(np.linalg.eigvalsh(A32.astype(np.float64)).min())
                out["degenerate"] = out["min_eig"] < prm["degenerate_eig"]
            six = (six + x).astype(F)
            dR = F(math.sqrt(sum(float(F(x[i] * F(57.29578))) ** 2 for i in range(3))))
            dT = F(math.sqrt(sum(float(F(x[i] * F(100.0))) ** 2 for i in range(3, 6))))
            out["last_deltas"] = (float(dR), float(dT))
            if float(dR) < prm["rot_conv_deg"] and float(dT) < prm["trans_conv_cm"]:
                out["converged"] = True
                break
    out["six"] = six
    out["pose"] = transformation(six).astype(np.float64)
    return out


def gate_margins(pp, prm=DEFAULTS):
    """The distance of every point to the gates it met, on the reference's own numbers: (n, 4) = |d2[4] - knn_max_sq|, |resid - plane_thresh|,
    |s - point_thresh|, d2[5] - d2[4] (inf where a gate was not reached; the tie only for points whose fifth neighbour passes)."""
    d5 = pp["d2"][:, 4].astype(np.float64)
    m = np.full((len(d5), 4), np.inf)
    m[:, 0] = np.abs(d5 - prm["knn_max_sq"])
    ok = np.isfinite(pp["resid"])
    m[ok, 1] = np.abs(pp["resid"][ok] - prm["plane_thresh"])
    ok = np.isfinite(pp["s"])
    m[ok, 2] = np.abs(pp["s"][ok].astype(np.float64) - prm["point_thresh"])
    near = d5 < prm["knn_max_sq"]
    m[near, 3] = pp["d2"][near, 5].astype(np.float64) - d5[near]
    return m


def patch_condition(tgt, idx5):
    """2-norm condition numbers of the 5 x 3 neighbour matrices"""
    A = np.asarray(tgt, np.float64)[:, :3][idx5]
    sv = np.linalg.svd(A, compute_uv=False)
    return sv[:, 0] / sv[:, -1]
