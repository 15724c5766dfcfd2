"""fast_gicp's two settings in plain numpy: the five regularisations of a per-point covariance (fast_gicp_impl.hpp:263-293) and the two voxel
folds (fast_vgicp_voxel.hpp:79-122) -- the reference that csrc/cov_math.h (cov_from_neighbours<kReg>) and csrc/vgicp.hip (vgicp_voxel_kernel<kFold>) are
checked against.  Built on cov_ref (neighbours, the long-double scatter) and gicp_ref (the GICP pass and the LM driver); it edits neither.

regularize(S, method) works on the scatter S with np.linalg.eigh and closed forms:
    NONE S; MIN_EIG V diag(max(w, 1e-3)) V^T; NORMALIZED_MIN_EIG V diag(max(w / w_max, 1e-3)) V^T; PLANE I - (1 - 1e-3) n n^T (cov_ref's form);
    FROBENIUS V diag((w + 1e-3) f) V^T with f = sqrt(sum 1 / (w + 1e-3)^2), which is ((C + 1e-3 I)^-1 / |(C + 1e-3 I)^-1|_F)^-1.
regularize_alt is the same by another route: np.linalg.svd and U diag V^T as the reference's JacobiSVD branch reads it, np.linalg.inv twice and
np.linalg.norm for FROBENIUS.

fold(points, covs, res, mode) is the voxel map: ADDITIVE (and ADDITIVE_WEIGHTED, the same class in the vendored fast_gicp) the mean of the points
and of their covariances; MULTIPLICATIVE cov = (sum C_i^-1)^-1, mean = cov sum C_i^-1 p_i.  fold(..., alt=True) takes every sum in np.longdouble and
every inverse by cofactors in np.longdouble.

The measure everywhere: the largest entry difference of a matrix (or vector) over the largest entry of the reference's.
"""
import ctypes as C

import numpy as np

import cov_ref
import gicp_ref

NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = range(5)
ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE = range(3)
REG_NAMES = {NONE: "NONE", MIN_EIG: "MIN_EIG", NORMALIZED_MIN_EIG: "NORMALIZED_MIN_EIG", PLANE: "PLANE", FROBENIUS: "FROBENIUS"}
MODE_NAMES = {ADDITIVE: "ADDITIVE", ADDITIVE_WEIGHTED: "ADDITIVE_WEIGHTED", MULTIPLICATIVE: "MULTIPLICATIVE"}
NEW_REGS = (NONE, MIN_EIG, NORMALIZED_MIN_EIG, FROBENIUS)
LAMBDA = 1e-3

# Largest normalised difference of regularize() against regularize_alt() over every query of cov_ref.clouds() (none is `ambiguous`) -- measured by
# tests/test_gicp_settings_ref.py::test_regularisations_against_their_alternative_evaluation, which holds the measurement to twice these figures.
# NONE has no arithmetic after the scatter, so its second evaluation is of the scatter: scatter_f64(), the same sums in plain float64 in the
# order the reference takes them (mean, centred products, sum, divide), against the long-double ones.
# Per cloud (lattice, plane, tilted, line, far_plane, blob, lidar, two_planes, clump):
#   NONE                6.1e-16 2.7e-16 6.4e-17 4.3e-16 4.5e-16 6.5e-16 4.3e-16 4.1e-16 7.1e-16
#   MIN_EIG             3.2e-15 6.4e-16 2.7e-15 2.2e-15 3.1e-15 6.9e-15 3.2e-15 3.3e-15 2.6e-15
#   NORMALIZED_MIN_EIG  2.8e-15 6.0e-16 2.4e-15 2.2e-15 2.9e-15 6.9e-15 3.5e-15 2.7e-15 5.8e-15
#   FROBENIUS           2.3e-15 4.0e-16 1.0e-14 1.6e-15 6.1e-15 2.2e-15 6.2e-15 4.7e-15 2.0e-15
REF_REG_MAX = {NONE: 7.5e-16, MIN_EIG: 7.0e-15, NORMALIZED_MIN_EIG: 7.0e-15, FROBENIUS: 1.1e-14}
# The device runs the same f64 algorithm with its own eigen-solver, inverse, divide and square root: ten times the reference's own error, the
# convention of cov_ref.DEVICE_ERR_GAP_BOUND.
DEVICE_REG_BOUND = {k: 10 * v for k, v in REF_REG_MAX.items()}

# The same for the fold over cov_ref.fold_map() at resolutions 1.0 and 2.0 (the worse of the two): fold() on regularize()'s covariances against
# fold(alt=True) on regularize_alt()'s -- both evaluations of the whole chain, since a fold inherits what its covariances are uncertain by (PLANE's
# eigenvectors above all) -- (mean, cov) per (regularisation, voxel mode), measured by test_fold_against_its_alternative_evaluation.
# Measured, ADDITIVE / MULTIPLICATIVE:
#   NONE                mean 0 cov 2.2e-15 / mean 1.9e-15 cov 1.2e-15        MIN_EIG    mean 0 cov 2.3e-15 / mean 3.8e-15 cov 2.4e-15
#   NORMALIZED_MIN_EIG  mean 0 cov 1.8e-15 / mean 1.5e-15 cov 2.1e-15        PLANE      mean 0 cov 1.6e-15 / mean 5.6e-14 cov 6.5e-13
#   FROBENIUS           mean 0 cov 1.6e-14 / mean 1.3e-15 cov 1.6e-14
# An ADDITIVE mean agrees exactly between the two evaluations; its figure is the one rounding of the result, 2^-52.
_EPS = 2.0 ** -52
REF_FOLD_MAX = {
    (NONE, ADDITIVE): (_EPS, 2.3e-15), (NONE, MULTIPLICATIVE): (2.0e-15, 1.3e-15),
    (MIN_EIG, ADDITIVE): (_EPS, 2.4e-15), (MIN_EIG, MULTIPLICATIVE): (3.9e-15, 2.5e-15),
    (NORMALIZED_MIN_EIG, ADDITIVE): (_EPS, 1.9e-15), (NORMALIZED_MIN_EIG, MULTIPLICATIVE): (1.5e-15, 2.1e-15),
    (PLANE, ADDITIVE): (_EPS, 1.7e-15), (PLANE, MULTIPLICATIVE): (5.7e-14, 6.6e-13),
    (FROBENIUS, ADDITIVE): (_EPS, 1.6e-14), (FROBENIUS, MULTIPLICATIVE): (1.4e-15, 1.6e-14),
}
DEVICE_FOLD_BOUND = {k: (10 * v[0], 10 * v[1]) for k, v in REF_FOLD_MAX.items()}
# The fixed-scale fold (ADDITIVE over PLANE / NORMALIZED_MIN_EIG covariances, whose entries are at most 1: csrc/vgicp.hip) rounds every term to a
# multiple of 2^-44 before it adds them exactly: by the format alone a mean and a mean covariance entry lie within 2^-45 of the exact ones.
# An absolute term, added to the bound above for those two pairs only.
FIXED_FOLD_QUANTUM = 2.0 ** -45
FIXED_FOLD = ((PLANE, ADDITIVE), (NORMALIZED_MIN_EIG, ADDITIVE))

# One linearisation per (regularisation, voxel mode) on fold_map() / fold_scan() at resolution 1.0 and fold_poses()[1]: linearize() on fold()
# against linearize() on fold(alt=True) with regularize_alt's covariances, cov_ref.lin_diff's (H, b, err) -- measured by
# test_linearisation_against_its_alternative_evaluation.  Measured (H b err), ADDITIVE / MULTIPLICATIVE:
#   NONE                8.0e-17 3.8e-16 3.8e-16 / 0 2.3e-14 5.3e-16          MIN_EIG    1.1e-16 2.0e-15 1.9e-16 / 1.5e-16 4.0e-14 0
#   NORMALIZED_MIN_EIG  2.5e-16 1.1e-15 1.9e-16 / 3.3e-16 3.5e-14 2.7e-16    PLANE      1.3e-13 4.1e-13 3.8e-15 / 2.8e-14 3.5e-13 1.0e-15
#   FROBENIUS           3.8e-16 1.2e-15 4.7e-16 / 3.5e-16 5.1e-14 1.0e-15
# On this map every eigenvalue is above 1e-3, so both routes return nearly the same covariances and several figures are accidents of a few
# ulps.  No figure is taken below LIN_SUM_FLOOR = 307 * 2^-53, the bound of one float64 summation of the 307 corresponding points' terms in
# whatever order ((n - 1) u sum |x|, Higham 4.4): another order of the same sum is as legitimate an evaluation as numpy's.
LIN_SUM_FLOOR = 307 * 2.0 ** -53
_LIN_MEASURED = {
    (NONE, ADDITIVE): (8.1e-17, 3.9e-16, 3.9e-16), (NONE, MULTIPLICATIVE): (0.0, 2.3e-14, 5.3e-16),
    (MIN_EIG, ADDITIVE): (1.1e-16, 2.1e-15, 2.0e-16), (MIN_EIG, MULTIPLICATIVE): (1.5e-16, 4.1e-14, 0.0),
    (NORMALIZED_MIN_EIG, ADDITIVE): (2.5e-16, 1.1e-15, 1.9e-16), (NORMALIZED_MIN_EIG, MULTIPLICATIVE): (3.4e-16, 3.5e-14, 2.8e-16),
    (PLANE, ADDITIVE): (1.3e-13, 4.2e-13, 3.8e-15), (PLANE, MULTIPLICATIVE): (2.8e-14, 3.5e-13, 1.1e-15),
    (FROBENIUS, ADDITIVE): (3.8e-16, 1.2e-15, 4.7e-16), (FROBENIUS, MULTIPLICATIVE): (3.5e-16, 5.2e-14, 1.1e-15),
}
REF_LIN_MAX = {k: tuple(max(x, LIN_SUM_FLOOR) for x in v) for k, v in _LIN_MEASURED.items()}
DEVICE_LIN_BOUND = {k: tuple(10 * x for x in v) for k, v in REF_LIN_MAX.items()}

# NONE leaves a singular scatter singular: whatever inverts NONE covariances uses clouds whose every query has w_min / w_max >= this
COND_FLOOR = 1e-6
WELL_CONDITIONED = ("blob", "lidar", "clump")


def scatter(pts, queries=None, k=cov_ref.K):
    """-> (S (m, 3, 3) float64: cov_ref's long-double scatter of the k neighbours, rounded once; the CovRef of the same queries)"""
    P = cov_ref._xyz32(pts)
    ref = cov_ref.covariances(P, queries, k)
    nb = P[ref.idx].astype(np.longdouble)
    c = nb - (nb.sum(axis=1) / np.longdouble(k))[:, None, :]
    S = ((c[:, :, :, None] * c[:, :, None, :]).sum(axis=1) / np.longdouble(k)).astype(np.float64)
    return S, ref


def scatter_f64(pts, idx, k=cov_ref.K):
    """the scatter of the neighbour lists idx in plain float64, in the order the reference takes it (fast_gicp_impl.hpp:255-261)"""
    nb = cov_ref._xyz32(pts)[idx].astype(np.float64)
    mean = np.zeros((nb.shape[0], 3))
    for j in range(k):
        mean += nb[:, j]
    c = nb - (mean / k)[:, None, :]
    S = np.zeros((nb.shape[0], 3, 3))
    for j in range(k):
        S += c[:, j, :, None] * c[:, j, None, :]
    return S / k


def _vdv(V, val):
    return np.einsum("nik,nk,njk->nij", V, val, V)


def regularize(S, method):
    S = np.asarray(S, np.float64)
    if method == NONE:
        return S.copy()
    w, V = np.linalg.eigh(S)
    if method == PLANE:
        n = V[:, :, 0]
        return np.eye(3)[None] - (1.0 - 1e-3) * n[:, :, None] * n[:, None, :]
    if method == MIN_EIG:
        return _vdv(V, np.maximum(w, 1e-3))
    if method == NORMALIZED_MIN_EIG:
        with np.errstate(all="ignore"):
            return _vdv(V, np.maximum(w / w[:, 2:3], 1e-3))
    if method == FROBENIUS:
        d = w + LAMBDA
        return _vdv(V, d * np.sqrt((1.0 / d ** 2).sum(axis=1))[:, None])
    raise ValueError(method)


def regularize_alt(S, method):
    S = np.asarray(S, np.float64)
    if method == NONE:
        return S.copy()
    if method == FROBENIUS:
        Ci = np.linalg.inv(S + LAMBDA * np.eye(3)[None])
        return np.linalg.inv(Ci / np.linalg.norm(Ci, axis=(1, 2))[:, None, None])
    U, sv, Vt = np.linalg.svd(S)
    if method == PLANE:
        val = np.broadcast_to(np.array([1.0, 1.0, 1e-3]), sv.shape)
    elif method == MIN_EIG:
        val = np.maximum(sv, 1e-3)
    elif method == NORMALIZED_MIN_EIG:
        with np.errstate(all="ignore"):
            val = np.maximum(sv / sv[:, :1], 1e-3)
    else:
        raise ValueError(method)
    # U = V for a symmetric positive semi-definite matrix, as the device's PLANE path already reads JacobiSVD
    return np.einsum("nik,nk,njk->nij", U, val, U)


def rel_diff(got, ref):
    """per matrix (or vector): the largest entry difference over the largest entry of the reference's"""
    got, ref = np.asarray(got), np.asarray(ref)
    ax = tuple(range(1, ref.ndim))
    scale = np.abs(ref).max(axis=ax)
    with np.errstate(all="ignore"):
        return np.where(scale > 0, np.abs(got - ref).max(axis=ax) / scale, np.abs(got - ref).max(axis=ax))


def conditioning(S):
    """w_min / w_max of every scatter"""
    w = np.linalg.eigvalsh(np.asarray(S, np.float64))
    with np.errstate(all="ignore"):
        return np.where(w[:, 2] > 0, w[:, 0] / w[:, 2], 0.0)


# ---------------------------------------------------------------------------
# the voxel map
# ---------------------------------------------------------------------------
def _inv_ld(S):
    """3x3 inverses by cofactors in np.longdouble"""
    L = np.asarray(S).astype(np.longdouble)
    a, b, c, d, e, f = L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]
    A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * A + b * B + c * Cc
    return np.stack([A, B, Cc, B, a * f - c * c, b * c - a * e, Cc, b * c - a * e, a * d - b * b], 1).reshape(-1, 3, 3) / det[:, None, None]


def fold(points, covs, res, mode, alt=False):
    """-> dict(ijk (m, 3) int64 sorted by (ix, iy, iz), n (m,), mean (m, 3), cov (m, 3, 3), rows: the rows of each voxel)"""
    P = cov_ref._xyz32(points).astype(np.float64)
    covs = np.asarray(covs, np.float64)
    ijk, inv = np.unique(cov_ref.voxel_coords(P, res), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    m = len(ijk)
    rows = [np.flatnonzero(inv == v) for v in range(m)]
    n = np.array([len(r) for r in rows])
    mean, cov = np.zeros((m, 3)), np.zeros((m, 3, 3))
    ft = np.longdouble if alt else np.float64
    with np.errstate(all="ignore"):
        for v, r in enumerate(rows):
            p, Cv = P[r].astype(ft), covs[r].astype(ft)
            if mode in (ADDITIVE, ADDITIVE_WEIGHTED):
                mean[v] = (p.sum(axis=0) / ft(len(r))).astype(np.float64)
                cov[v] = (Cv.sum(axis=0) / ft(len(r))).astype(np.float64)
            elif mode == MULTIPLICATIVE:
                if alt:
                    A = _inv_ld(Cv)
                    Sg = _inv_ld(A.sum(axis=0)[None])[0]
                else:
                    A = np.linalg.inv(Cv)
                    Sg = np.linalg.inv(A.sum(axis=0))
                cov[v] = Sg.astype(np.float64)
                mean[v] = (Sg @ np.einsum("nij,nj->i", A, p)).astype(np.float64)
            else:
                raise ValueError(mode)
    return dict(ijk=ijk.astype(np.int64), n=n, mean=mean, cov=cov, rows=rows)


def linearize(scan, pose, src_cov, voxels, res=1.0):
    """cov_ref.linearize with the voxel map given (fold()): the voxel mode is the fold's -> dict(H, b, err, n)"""
    scan = np.asarray(scan)
    table = {tuple(c): v for v, c in enumerate(voxels["ijk"])}
    H, b, err, nc = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    R, t = pose[:3, :3], pose[:3, 3]
    for i in range(scan.shape[0]):
        tp = R @ scan[i, :3].astype(np.float64) + t
        v = table.get(tuple(np.floor(tp / res - 0.5).astype(int)))
        if v is None:
            continue
        M = np.linalg.inv(voxels["cov"][v] + R @ src_cov[i] @ R.T)
        e = voxels["mean"][v] - tp
        w = np.sqrt(voxels["n"][v])
        Sk = np.array([[0, -tp[2], tp[1]], [tp[2], 0, -tp[0]], [-tp[1], tp[0], 0]])
        J = np.concatenate([Sk, -np.eye(3)], 1)
        H += w * J.T @ M @ J; b += w * J.T @ M @ e; err += w * e @ M @ e; nc += 1
    return dict(H=H, b=b, err=float(err), n=nc)


def _lin_state(scan, pose, src_cov, voxels, res):
    """linearize() that also keeps the correspondences: (sums, [(i, voxel, M)])"""
    scan = np.asarray(scan)
    table = {tuple(c): v for v, c in enumerate(voxels["ijk"])}
    R, t = pose[:3, :3], pose[:3, 3]
    tp = scan[:, :3].astype(np.float64) @ R.T + t
    key = np.floor(tp / res - 0.5).astype(int)
    vi = np.array([table.get(tuple(c), -1) for c in key])
    has = np.flatnonzero(vi >= 0)
    v = vi[has]
    M = np.linalg.inv(voxels["cov"][v] + R @ src_cov[has] @ R.T)
    e = voxels["mean"][v] - tp[has]
    w = np.sqrt(voxels["n"][v].astype(np.float64))
    x = tp[has]
    J = np.zeros((len(has), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -x[:, 2], x[:, 1], x[:, 2], -x[:, 0], -x[:, 1], x[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    Me = np.einsum("nij,nj->ni", M, e)
    H = np.einsum("n,nki,nkl,nlj->ij", w, J, M, J)
    b = np.einsum("n,nki,nk->i", w, J, Me)
    err = float((w * np.einsum("ni,ni->n", e, Me)).sum())
    return dict(H=H, b=b, err=err, n=len(has)), (has, v, M, w)


def vgicp_align(scan, voxels, guess, src_cov, res=1.0, max_iters=64, lm_inner=10, lm_init_scale=1e-9, rot_eps=2e-3, trans_eps=5e-4):
    """-> dict(pose, converged, outer, passes): the library's host-only LM state machine (pcr_vgicp_opt_*) fed with this module's VGICP sums, as
    gicp_ref.align feeds it GICP's.  compute_error (fast_vgicp_impl.hpp:183-204): the correspondences and matrices of the last linearisation."""
    from simpleslam_amd.pcr import load_library
    L = load_library()
    dp = C.POINTER(C.c_double)
    scan = np.asarray(scan)
    g = np.ascontiguousarray(np.asarray(guess, np.float64).T).reshape(16).copy()
    o = L.pcr_vgicp_opt_create(g.ctypes.data_as(dp), int(max_iters), int(lm_inner), float(lm_init_scale), float(rot_eps), float(trans_eps))
    assert o
    cache = {}

    def lin(T):
        k = T.tobytes()
        if k not in cache:
            if len(cache) == 2:
                del cache[next(iter(cache))]
            cache[k] = _lin_state(scan, T, src_cov, voxels, res)
        return cache[k]

    try:
        passes = 0
        for _ in range(max_iters * max(1, lm_inner) + 3):
            kind, pe, pl = C.c_int(-1), np.zeros(16), np.zeros(16)
            assert L.pcr_vgicp_opt_request(o, C.byref(kind), pe.ctypes.data_as(dp), pl.ctypes.data_as(dp)) == 0
            if kind.value == 2:
                break
            Te, Tl = pe.reshape(4, 4).T.copy(), pl.reshape(4, 4).T.copy()
            sums = np.zeros(29)
            if kind.value == 1:
                has, v, M, w = lin(Tl)[1]
                e = voxels["mean"][v] - (scan[has, :3].astype(np.float64) @ Te[:3, :3].T + Te[:3, 3])
                sums[28] = float((w * np.einsum("ni,nij,nj->n", e, M, e)).sum())
            r = lin(Te)[0]
            sums[:21] = r["H"][np.triu_indices(6)]
            sums[21:27] = r["b"]
            sums[27] = r["err"]
            assert L.pcr_vgicp_opt_feed(o, sums.ctypes.data_as(dp)) == 0
            passes += 1
        else:
            raise AssertionError("the optimiser did not finish")
        pose, conv, outer, done = np.zeros(16), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.pcr_vgicp_opt_result(o, pose.ctypes.data_as(dp), C.byref(conv), C.byref(outer), C.byref(done)) == 0 and done.value == 1
    finally:
        L.pcr_vgicp_opt_destroy(o)
    return dict(pose=pose.reshape(4, 4).T.astype(np.float32).astype(np.float64), converged=bool(conv.value), outer=outer.value, passes=passes)


gicp_align = gicp_ref.align      # (GICP: gicp_ref's driver serves as it is, given C_A and C_B of the regularisation)
