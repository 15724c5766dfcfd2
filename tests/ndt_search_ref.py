"""An independent reference for NDT's neighbourhood settings (pcr_params.ndt_search): DIRECT1, DIRECT7 and DIRECT26.

oracle/ndt_oracle.c knows DIRECT7 only.  This module restates, in numpy and with no code of csrc/, what pclomp does per (point, voxel)
pair -- computePointDerivatives / updateDerivatives in float32 in the reference's operation order (ndt_omp_impl.hpp:399-440, :485-537),
the double updateHessian (:444-481, :614-645) -- around a lookup with the three offset tables (voxel_grid_covariance_omp_impl.hpp:374-441).
The voxel Gaussians are the oracle's own (oracle.ndt_leaves); expf, sinf and cosf are the C library's, called through ctypes (the
project's exact NDT parity rests on the C library's expf).  Pairs are summed in float64.  tests/test_ndt_search_ref.py holds this module
to the oracle under DIRECT7.

DIRECT26 is pcl::getAllNeighborCellIndices(): the 13 cells of the half neighbourhood -- (i, j, -1) for i, j in -1..1 with i outermost,
then (i, -1, 0) for i in -1..1, then (-1, 0, 0) -- followed by their negations: 26 cells, the centre excluded.  (Restated from PCL
1.8 - 1.12 as remembered; see DESIGN.md.)"""
import ctypes as C
import ctypes.util

import numpy as np

import oracle

KDTREE, DIRECT26, DIRECT7, DIRECT1 = range(4)
NAMES = {DIRECT26: "DIRECT26", DIRECT7: "DIRECT7", DIRECT1: "DIRECT1"}

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in ("expf", "sinf", "cosf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]

F = np.float32


def _expf(x):
    return np.array([_libm.expf(float(v)) for v in np.asarray(x, F).ravel()], F).reshape(np.shape(x))


def offsets(search):
    """the offset table of a setting, in the reference's visiting order: (k, 3) int"""
    if search == DIRECT1:
        return np.array([[0, 0, 0]])
    if search == DIRECT7:
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    if search == DIRECT26:
        half = [(i, j, -1) for i in (-1, 0, 1) for j in (-1, 0, 1)] + [(i, -1, 0) for i in (-1, 0, 1)] + [(-1, 0, 0)]
        return np.array(half + [(-a, -b, -c) for a, b, c in half])
    raise ValueError(f"no offset table for ndt_search = {search}")


class Target:
    """the kept voxels of a target and its lattice box, as VoxelGridCovariance holds them"""

    def __init__(self, dst, prm=None):
        self.prm = prm or oracle.ndt_params()
        self.leaf = F(self.prm.resolution)
        dst = np.asarray(dst, F)
        lv = oracle.ndt_leaves(dst, self.prm)
        keep = lv["n"] >= max(3, int(self.prm.min_points))       # (-1: rejected by the eigenvalue or the inverse test)
        self.mean, self.icov = lv["mean"][keep], lv["icov"][keep]
        self.index = {tuple(int(v) for v in c): k for k, c in enumerate(lv["ijk"][keep])}
        xyz = dst[:, :3][np.isfinite(dst[:, :3]).all(1)]
        inv = F(1.0) / self.leaf
        if len(xyz):      # min_b / max_b: floor(min_p * inverse_leaf) in float (voxel_grid_covariance_omp_impl.hpp:90-95)
            self.min_b = np.floor(xyz.min(0) * inv).astype(np.int64)
            self.max_b = np.floor(xyz.max(0) * inv).astype(np.int64)
        else:
            self.min_b, self.max_b = np.zeros(3, np.int64), -np.ones(3, np.int64)
        res = float(self.leaf)
        c1, c2 = 10 * (1 - self.prm.outlier_ratio), self.prm.outlier_ratio / res ** 3      # ndt_omp_impl.hpp:86-93
        d3 = -np.log(c2)
        self.d1 = -np.log(c1 + c2) - d3
        self.d2 = -2 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / self.d1)

    def pairs(self, tp, search):
        """(point index, voxel index) of every pair, point by point in the table's order"""
        cells = np.floor(tp / self.leaf).astype(np.int64)       # float division, as :380-382
        pi, vi = [], []
        for i, c in enumerate(cells):
            for d in offsets(search):
                q = c + d
                if (q >= self.min_b).all() and (q <= self.max_b).all():
                    k = self.index.get((int(q[0]), int(q[1]), int(q[2])))
                    if k is not None:
                        pi.append(i); vi.append(k)
        return np.array(pi, np.int64), np.array(vi, np.int64)


def _axis_rot(angle, axis):
    """Eigen::AngleAxisf(angle, Unit).toRotationMatrix() in float"""
    s, c = F(_libm.sinf(float(F(angle)))), F(_libm.cosf(float(F(angle))))
    ax = np.zeros(3, F); ax[axis] = 1
    sa, c1 = s * ax, (F(1) - c) * ax
    R = np.zeros((3, 3), F)
    t = c1[0] * ax[1]; R[0, 1] = t - sa[2]; R[1, 0] = t + sa[2]
    t = c1[0] * ax[2]; R[0, 2] = t + sa[1]; R[2, 0] = t - sa[1]
    t = c1[1] * ax[2]; R[1, 2] = t - sa[0]; R[2, 1] = t + sa[0]
    for d in range(3):
        R[d, d] = c1[d] * ax[d] + c
    return R


def _mul33(A, B):
    out = np.zeros((3, 3), F)
    for r in range(3):
        for c in range(3):
            s = A[r, 0] * B[0, c]; s = s + A[r, 1] * B[1, c]; s = s + A[r, 2] * B[2, c]
            out[r, c] = s
    return out


def pose_from_p(p6):
    """Translation * Rx * Ry * Rz in float (ndt_omp_impl.hpp:146-149) -> (R float32 3x3, t float32 3)"""
    R = _mul33(_mul33(_axis_rot(p6[3], 0), _axis_rot(p6[4], 1)), _axis_rot(p6[5], 2))
    return R, np.asarray(p6[:3], np.float64).astype(F)


def pose16_to_Rt(pose):
    P = np.asarray(pose, np.float64).reshape(4, 4).astype(F)
    return P[:3, :3].copy(), P[:3, 3].copy()


def angle_tables(p6):
    """computeAngleDerivatives (:289-395): the double vectors and the float tables (whose row 6 holds +sy where the double d1 holds -sy)"""
    def sc(a):
        return (0.0, 1.0) if abs(a) < 10e-5 else (np.sin(a), np.cos(a))
    (sx, cx), (sy, cy), (sz, cz) = sc(p6[3]), sc(p6[4]), sc(p6[5])
    J = np.array([[-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy], [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy],
                  [-sy * cz, sy * sz, cy], [sx * cy * cz, -sx * cy * sz, sx * sy], [-cx * cy * cz, cx * cy * sz, -cx * sy],
                  [-cy * sz, -cy * cz, 0], [cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0], [sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0]])
    H = np.array([[-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy], [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy],
                  [cx * cy * cz, -cx * cy * sz, cx * sy], [sx * cy * cz, -sx * cy * sz, sx * sy],
                  [-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0], [cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0],
                  [-cy * cz, cy * sz, -sy], [-sx * sy * cz, sx * sy * sz, sx * cy], [cx * sy * cz, -cx * sy * sz, -cx * cy],
                  [sy * sz, sy * cz, 0], [-sx * cy * sz, -sx * cy * cz, 0], [cx * cy * sz, cx * cy * cz, 0],
                  [-cy * cz, cy * sz, 0], [-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0], [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0]])
    Hf = H.astype(F)
    Hf[6, 2] = F(sy)
    return J, H, J.astype(F), Hf


def _dot3(a, b):
    """sum_k a[k] * b[k], k = 0, 1, 2, left to right in the arrays' own precision; a, b: sequences of three arrays"""
    s = a[0] * b[0]
    s = s + a[1] * b[1]
    return s + a[2] * b[2]


# the second derivative of the transform for parameters (3 + a, 3 + b): which of the vectors a..f of :421-438
_PH = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]


def transform(scan, R, t):
    """pcl::transformPointCloud in float"""
    x = np.asarray(scan, F)[:, :3]
    tp = np.zeros_like(x)
    for r in range(3):
        s = R[r, 0] * x[:, 0]; s = s + R[r, 1] * x[:, 1]; s = s + R[r, 2] * x[:, 2]
        tp[:, r] = s + t[r]
    return tp


def sums(target, scan, p6, search, kind=0, Rt=None, tile=None):
    """One pass at p6: kind 0 = computeDerivatives with the float Hessian, 1 = without it, 2 = computeHessian (double).
    -> dict(score, grad, hess | hess_d, pairs).  Rt: the float transform when it is not the one p6 gives (the optimiser hands over its
    own); tile = (lo, hi): only points whose transformed position lies in [lo, hi)."""
    p6 = np.asarray(p6, np.float64)
    R, t = Rt if Rt is not None else pose_from_p(p6)
    x = np.asarray(scan, F)[:, :3]
    tp = transform(scan, R, t)
    pi, vi = target.pairs(tp, search)
    if tile is not None and len(pi):
        tpd = tp.astype(np.float64)[pi]
        ok = ((tpd >= np.asarray(tile[0])) & (tpd < np.asarray(tile[1]))).all(1)
        pi, vi = pi[ok], vi[ok]
    out = dict(pairs=len(pi))
    Jd, Hd, Jf, Hf = angle_tables(p6)
    if len(pi) == 0:
        z = dict(score=0.0, grad=np.zeros(6), hess=np.zeros((6, 6)))
        out.update({0: z, 1: dict(score=0.0, grad=np.zeros(6)), 2: dict(hess_d=np.zeros((6, 6)))}[kind])
        return out
    xt = tp.astype(np.float64)[pi] - target.mean[vi]                # x_trans -= mean, in double
    icov = target.icov[vi]
    d1, d2 = target.d1, target.d2
    if kind == 2:
        xp = x.astype(np.float64)[pi]
        pg = np.zeros((len(pi), 3, 6)); pg[:, 0, 0] = pg[:, 1, 1] = pg[:, 2, 2] = 1.0
        dj = xp @ Jd.T
        for k, (r, c) in enumerate([(1, 3), (2, 3), (0, 4), (1, 4), (2, 4), (0, 5), (1, 5), (2, 5)]):
            pg[:, r, c] = dj[:, k]
        dh = xp @ Hd.T
        z = np.zeros(len(pi))
        vec = [np.stack([z, dh[:, 0], dh[:, 1]], 1), np.stack([z, dh[:, 2], dh[:, 3]], 1), np.stack([z, dh[:, 4], dh[:, 5]], 1),
               dh[:, 6:9], dh[:, 9:12], dh[:, 12:15]]
        cx = np.einsum("nrc,nc->nr", icov, xt)
        e = d2 * np.exp(-d2 * np.einsum("nr,nr->n", xt, cx) / 2)
        ok = ~((e > 1) | (e < 0) | (e != e))
        e = e * d1
        cpg = np.einsum("nrc,nci->nri", icov, pg)                   # c_inv * point_gradient.col(i)
        xd = np.einsum("nr,nri->ni", xt, cpg)
        Hs = np.zeros((6, 6))
        for i in range(6):
            for j in range(6):
                term = -d2 * xd[:, i] * xd[:, j]
                if i >= 3 and j >= 3:
                    term = term + np.einsum("nr,nr->n", xt, np.einsum("nrc,nc->nr", icov, vec[_PH[i - 3][j - 3]]))
                term = term + np.einsum("nr,nr->n", pg[:, :, j], cpg[:, :, i])
                Hs[i, j] = (e * term)[ok].sum()
        out["hess_d"] = Hs
        return out
    # ---- float: computePointDerivatives (:399-440)
    xs = x[pi]
    x4 = [xs[:, 0], xs[:, 1], xs[:, 2]]
    pg = [[np.full(len(pi), F(1.0 if r == c else 0.0)) for c in range(6)] for r in range(3)]
    xj = [_dot3(Jf[k], x4) for k in range(8)]
    for k, (r, c) in enumerate([(1, 3), (2, 3), (0, 4), (1, 4), (2, 4), (0, 5), (1, 5), (2, 5)]):
        pg[r][c] = xj[k]
    xh = [_dot3(Hf[k], x4) for k in range(15)]
    zf = np.zeros(len(pi), F)
    vec = [[zf, xh[0], xh[1]], [zf, xh[2], xh[3]], [zf, xh[4], xh[5]], [xh[6], xh[7], xh[8]], [xh[9], xh[10], xh[11]], [xh[12], xh[13], xh[14]]]
    # ---- updateDerivatives (:485-537)
    x4t = [xt[:, k].astype(F) for k in range(3)]
    ci = [[icov[:, r, c].astype(F) for c in range(3)] for r in range(3)]
    gd2 = F(d2)
    xc = [_dot3(x4t, [ci[0][c], ci[1][c], ci[2][c]]) for c in range(3)]             # x_trans4 * c_inv4
    e = _expf(-gd2 * _dot3(x4t, xc) * F(0.5))
    score_inc = (-d1 * e.astype(np.float64)).astype(F)
    e = gd2 * e
    ok = ~((e > 1) | (e < 0) | (e != e))
    e = (e.astype(np.float64) * d1).astype(F)
    cpg = [[_dot3(ci[r], [pg[0][c], pg[1][c], pg[2][c]]) for c in range(6)] for r in range(3)]      # c_inv4 * point_gradient4
    xcpg = [_dot3(x4t, [cpg[0][c], cpg[1][c], cpg[2][c]]) for c in range(6)]
    assert all(a.dtype == F for a in xcpg) and e.dtype == F and score_inc.dtype == F
    out["score"] = float(score_inc[ok].astype(np.float64).sum())
    out["grad"] = np.array([(e * xcpg[c])[ok].astype(np.float64).sum() for c in range(6)])
    if kind == 0:
        Hs = np.zeros((6, 6))
        for i in range(6):
            for j in range(6):
                term = -gd2 * xcpg[i] * xcpg[j]
                if i >= 3 and j >= 3:
                    term = term + _dot3(xc, vec[_PH[i - 3][j - 3]])
                else:
                    term = term + zf
                term = term + _dot3([pg[0][j], pg[1][j], pg[2][j]], [cpg[0][i], cpg[1][i], cpg[2][i]])
                assert term.dtype == F
                Hs[i, j] = (e * term)[ok].astype(np.float64).sum()
        out["hess"] = Hs
    return out


def sums43(d, kind):
    s = np.zeros(43)
    if kind != 2:
        s[0] = d["score"]; s[1:7] = d["grad"]
    if kind == 0:
        s[7:] = d["hess"].reshape(36)
    if kind == 2:
        s[7:] = d["hess_d"].reshape(36)
    return s


def drive(evaluate, guess, prm=None, scale=1.0, limit=600):
    """The project's Newton / More-Thuente state machine (pcr_ndt_opt_*, host only) with every pass it asks for answered by
    evaluate(kind, p6, (R, t)) -> 43 sums (each multiplied by `scale`).  -> (pose 4x4, converged, iterations, passes)."""
    from simpleslam_amd.pcr import load_library
    L = load_library()
    prm = prm or oracle.ndt_params()
    dp = C.POINTER(C.c_double)
    g = np.ascontiguousarray(np.asarray(guess, np.float64).T).reshape(16).copy()
    o = L.pcr_ndt_opt_create(g.ctypes.data_as(dp), float(prm.step_size), float(prm.trans_eps), int(prm.max_iters))
    assert o
    try:
        passes = 0
        for _ in range(limit):
            kind, p6, pose = C.c_int(-1), np.zeros(6), np.zeros(16)
            assert L.pcr_ndt_opt_request(o, C.byref(kind), p6.ctypes.data_as(dp), pose.ctypes.data_as(dp)) == 0
            if kind.value == 3:
                break
            s = np.ascontiguousarray(evaluate(kind.value, p6, pose16_to_Rt(pose.reshape(4, 4).T)) * scale)
            assert L.pcr_ndt_opt_feed(o, s.ctypes.data_as(dp)) == 0
            passes += 1
        else:
            raise AssertionError("the optimiser did not finish")
        out, conv, its, done = np.zeros(16), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.pcr_ndt_opt_result(o, out.ctypes.data_as(dp), C.byref(conv), C.byref(its), C.byref(done)) == 0 and done.value == 1
    finally:
        L.pcr_ndt_opt_destroy(o)
    return out.reshape(4, 4).T.copy(), bool(conv.value), its.value, passes


def scan2map(target, scan, guess, search, scale=1.0):
    """the reference-driven optimiser under `search`"""
    return drive(lambda kind, p6, Rt: sums43(sums(target, scan, p6, search, kind, Rt=Rt), kind), guess, target.prm, scale)


# The end-to-end inputs of tests/test_ndt_search_gpu.py, checked on the CPU by tests/test_ndt_search_ref.py: the room of tests/ndt_clouds.py,
# 513 of its points with 1 cm of noise, and a guess drawn by synth.perturb(identity, seed, trans, rot_deg) from the seed recorded here.
E2E_SCAN = 513
E2E_GUESS = {DIRECT1: (4101, 0.25, 1.5), DIRECT26: (4105, 0.4, 2.5)}


def e2e_case(search):
    import ndt_clouds as nc
    from simpleslam_amd import synth
    m, scan, _ = nc.room_scan_case(E2E_SCAN)
    seed, trans, rot = E2E_GUESS[search]
    return m, scan, synth.perturb(np.eye(4), seed, trans=trans, rot_deg=rot)
