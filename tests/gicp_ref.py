"""Point-wise GICP (fast_gicp::FastGICP, fast_gicp_impl.hpp:103-237) in plain numpy: the reference the device's gicp pass is checked against.

One linearisation at pose T (float64), for every source point a_i with covariance C_A[i], against target points b_j with covariances C_B[j]:

- q = Tf a_i in float32 (fitness_ref.transform_f32), j = the target point with the smallest float32 squared distance (fitness_ref.nearest_sq:
  the lowest row among exact ties), d2 that distance;
- the gate: a correspondence needs d2 < thr2, thr2 = float32(max_dist) * float32(max_dist) formed in float32 (+inf by default); a source point
  with a coordinate that is not finite has none;
- M_i = (C_B[j] + R C_A[i] R^T)^-1, e = b_j - (R a_i + t), J = [skew(R a_i + t) | -I], all in float64;
- err = sum e^T M e, H = sum J^T M J, b = sum J^T M e; the twist is [rotation; translation].

error() is compute_error: a trial pose on the correspondences and matrices of an earlier linearisation.  align() drives the library's host-only
LM state machine (pcr_vgicp_opt_*, pinned to the oracle by tests/test_host.py) with these sums.

The covariances that go in come from cov_ref.covariances or oracle.vgicp_covariances.
"""
import ctypes as C
import functools
import math

import numpy as np

import fitness_ref

FLT_MAX = float(np.finfo(np.float32).max)

# Largest relative differences of this reference against a second evaluation of itself (alt_mahalanobis, alt_sums: M by np.linalg.inv of the
# reference's 4x4 form and by cofactors in np.longdouble, the sums by math.fsum) over world_small at the perturbed pose, at the truth and with the
# gate at 0.3 m -- measured by tests/test_gicp_ref.py::test_reference_against_its_alternative_evaluation, which holds the alternative to twice
# these figures.  M: largest entry difference over the largest entry of that matrix, worst matrix; H, b: cov_ref.lin_diff's convention (largest
# entry difference over the largest entry); err: relative.  Measured (perturbed / truth / gated): M by the 4x4 inverse 3.1e-16 / 3.4e-16 / 2.0e-16,
# by long-double cofactors 1.4e-14 / 1.7e-14 / 1.4e-14; H 4.0e-15 / 5.2e-15 / 7.8e-16; b 1.2e-16 / 2.4e-15 / 1.7e-15; err 1.6e-16 / 2.0e-16 / 1.5e-16.
REF_M_MAX = 1.8e-14
REF_H_MAX = 5.2e-15
REF_B_MAX = 2.4e-15
REF_ERR_MAX = 2.1e-16
# The device evaluates the same formulas with its own inverse (cofactors), divide and summation order: ten times the reference's own error,
# the convention of cov_ref.py.
DEVICE_M_BOUND = 10 * REF_M_MAX
DEVICE_H_BOUND = 10 * REF_H_MAX
DEVICE_B_BOUND = 10 * REF_B_MAX
DEVICE_ERR_BOUND = 10 * REF_ERR_MAX


@functools.lru_cache(maxsize=None)
def world_small_case():
    """conftest's world_small (8 192-point scan, 30 000-point map, perturbed by 0.2 m / 1 degree) with the oracle's covariances of both clouds:
    computed once, shared by the tests, never written to"""
    import oracle
    from simpleslam_amd import synth
    world, m = synth.make_map(30_000, seed=5)
    scan, T = synth.make_scan(world, 0, seed=5, beams=16, azimuths=512)
    w = dict(map=m, scan=scan, truth=T, init=synth.perturb(T, 5, trans=0.2, rot_deg=1.0),
             C_A=oracle.vgicp_covariances(scan, threads=8), C_B=oracle.vgicp_covariances(m, threads=8))
    for v in w.values():
        v.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def world_small_alignment():
    """align() on world_small_case() with the reference's default parameters"""
    w = world_small_case()
    return align(w["scan"], w["map"], w["init"], w["C_A"], w["C_B"])


def lattice_case():
    """a 6 x 6 x 6 unit lattice and the midpoints of its x-edges: every query has exactly two nearest points, one unit apart in x"""
    g = np.arange(6, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    dst = np.zeros((216, 4), np.float32)
    dst[:, 0], dst[:, 1], dst[:, 2] = x.ravel(), y.ravel(), z.ravel()
    lo = dst[dst[:, 0] < 5]
    src = lo.copy()
    src[:, 0] += 0.5
    want = np.array([np.nonzero((dst[:, :3] == p[:3]).all(axis=1))[0][0] for p in lo])
    return src, dst, want


def _xyz64(cloud):
    return fitness_ref._xyz(cloud).astype(np.float64)


def thr2_of(max_dist):
    with np.errstate(over="ignore"):
        return np.float32(max_dist) * np.float32(max_dist)


def second_nearest_sq(q, dst, idx, chunk_elems=1 << 22):
    """Float32 squared distance from each query to the nearest finite target point OTHER than row idx[i] (inf when there is none)."""
    t_all = fitness_ref._xyz(dst)
    rows = np.nonzero(np.isfinite(t_all).all(axis=1))[0]
    t = t_all[rows]
    out = np.full(q.shape[0], np.inf, np.float32)
    if t.shape[0] < 2:
        return out
    col = np.searchsorted(rows, idx)
    step = max(1, chunk_elems // t.shape[0])
    with np.errstate(all="ignore"):
        for a in range(0, q.shape[0], step):
            d = fitness_ref.sq_dist_f32(q[a:a + step], t)
            d = np.where(np.isnan(d), np.float32(np.inf), d)
            ok = idx[a:a + step] >= 0
            d[np.nonzero(ok)[0], col[a:a + step][ok]] = np.inf
            out[a:a + step] = d.min(axis=1)
    return out


def correspondences(src, dst, pose, max_dist=FLT_MAX, with_ambiguous=True):
    """-> corr (n,) int64, -1 for none; d2 (n,) float32, +inf for none; ambiguous (n,) bool: the nearest and the second-nearest float distances
    are unequal but within one float ulp (another rounding of the same distances could choose the other point)."""
    q = fitness_ref.transform_f32(src, pose)
    d2, idx = fitness_ref.nearest_sq(q, dst)
    finite = np.isfinite(fitness_ref._xyz(src)).all(axis=1)
    with np.errstate(invalid="ignore"):
        ok = finite & (idx >= 0) & (d2 < thr2_of(max_dist))
    amb = np.zeros(q.shape[0], bool)
    if with_ambiguous:
        d2b = second_nearest_sq(q, dst, idx)
        with np.errstate(invalid="ignore"):
            amb = finite & (idx >= 0) & (d2b != d2) & (d2b <= np.nextafter(d2, np.float32(np.inf)))
    return np.where(ok, idx, -1), np.where(ok, d2, np.float32(np.inf)).astype(np.float32), amb


def _fused(C_A, C_B, pose, corr):
    has = corr >= 0
    R = np.asarray(pose, np.float64)[:3, :3]
    return has, C_B[corr[has]] + R @ C_A[has] @ R.T


def mahalanobis(C_A, C_B, pose, corr):
    """(n, 3, 3) float64: (C_B[j] + R C_A[i] R^T)^-1, zeros where corr is -1."""
    has, S = _fused(C_A, C_B, pose, corr)
    M = np.zeros((corr.shape[0], 3, 3))
    M[has] = np.linalg.inv(S)
    return M


def _terms(src, dst, pose, corr, M):
    has = corr >= 0
    T = np.asarray(pose, np.float64)
    a = _xyz64(src)[has]
    tp = np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] for r in range(3)], 1)
    e = _xyz64(dst)[corr[has]] - tp
    return has, tp, e, M[has]


def _per_point(src, dst, pose, corr, M):
    """per corresponding point: J^T M J (k, 6, 6), J^T M e (k, 6), e^T M e (k,)"""
    has, tp, e, Mh = _terms(src, dst, pose, corr, M)
    J = np.zeros((tp.shape[0], 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -tp[:, 2], tp[:, 1], tp[:, 2], -tp[:, 0], -tp[:, 1], tp[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    Me = np.einsum("nij,nj->ni", Mh, e)
    return np.einsum("nki,nkl,nlj->nij", J, Mh, J), np.einsum("nki,nk->ni", J, Me), np.einsum("ni,ni->n", e, Me)


def linearize(src, dst, pose, C_A, C_B, max_dist=FLT_MAX, with_ambiguous=False):
    """-> dict(H, b, err, n, corr, d2, M, ambiguous)"""
    corr, d2, amb = correspondences(src, dst, pose, max_dist, with_ambiguous)
    M = mahalanobis(C_A, C_B, pose, corr)
    Hn, bn, en = _per_point(src, dst, pose, corr, M)
    return dict(H=Hn.sum(axis=0), b=bn.sum(axis=0), err=float(en.sum()), n=int((corr >= 0).sum()), corr=corr, d2=d2, M=M, ambiguous=amb)


def error(src, dst, pose_eval, corr, M):
    """compute_error: sum of e^T M e at pose_eval on the correspondences and matrices of an earlier linearisation"""
    _, _, e, Mh = _terms(src, dst, pose_eval, corr, M)
    return float(np.einsum("ni,nij,nj->n", e, Mh, e).sum())


# ---- the second evaluation -------------------------------------------------------------------------------------------------------------
def alt_mahalanobis(C_A, C_B, pose, corr):
    """(M by np.linalg.inv of the reference's 4x4 form -- (3,3) set to 1, zeroed afterwards --, M by cofactors in np.longdouble)"""
    has, S = _fused(C_A, C_B, pose, corr)
    S4 = np.zeros((S.shape[0], 4, 4))
    S4[:, :3, :3] = S
    S4[:, 3, 3] = 1.0
    M4 = np.zeros((corr.shape[0], 3, 3))
    M4[has] = np.linalg.inv(S4)[:, :3, :3]
    L = S.astype(np.longdouble)
    a, b, c, d, e, f = L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]
    A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * A + b * B + c * Cc
    ML = np.zeros((corr.shape[0], 3, 3), np.longdouble)
    ML[has] = np.stack([A, B, Cc, B, a * f - c * c, b * c - a * e, Cc, b * c - a * e, a * d - b * b], 1).reshape(-1, 3, 3) / det[:, None, None]
    return M4, ML.astype(np.float64)


def alt_sums(src, dst, pose, corr, M):
    """(H, b, err) with every sum taken by math.fsum (exactly rounded) instead of numpy's pairwise order"""
    Hn, bn, en = _per_point(src, dst, pose, corr, M)
    H = np.array([[math.fsum(Hn[:, i, j]) for j in range(6)] for i in range(6)])
    return H, np.array([math.fsum(bn[:, i]) for i in range(6)]), math.fsum(en)


def m_diff(got, ref):
    """largest entry difference of a matrix over the largest entry of the reference's, maximum over the matrices that have one"""
    scale = np.abs(ref).max(axis=(1, 2))
    has = scale > 0
    return float((np.abs(got - ref).max(axis=(1, 2))[has] / scale[has]).max()) if has.any() else 0.0


def sums_diff(got, ref):
    """(dH, db, derr), cov_ref.lin_diff's convention"""
    return (float(np.abs(got["H"] - ref["H"]).max() / np.abs(ref["H"]).max()), float(np.abs(got["b"] - ref["b"]).max() / np.abs(ref["b"]).max()),
            float(abs(got["err"] - ref["err"]) / abs(ref["err"])))


# ---- the whole alignment ---------------------------------------------------------------------------------------------------------------
def align(src, dst, guess, C_A, C_B, max_iters=64, lm_inner=10, lm_init_scale=1e-9, rot_eps=2e-3, trans_eps=5e-4, max_dist=FLT_MAX):
    """-> dict(pose, converged, outer, passes): the library's LM state machine (csrc/vgicp_opt.h through pcr_vgicp_opt_*, host only) fed with
    this module's sums.  The guess goes in and the result comes out as a Matrix4f, as VgicpRegister hands them over."""
    from simpleslam_amd.pcr import load_library
    L = load_library()
    dp = C.POINTER(C.c_double)
    g = np.ascontiguousarray(np.asarray(guess, np.float64).T).reshape(16).copy()
    o = L.pcr_vgicp_opt_create(g.ctypes.data_as(dp), int(max_iters), int(lm_inner), float(lm_init_scale), float(rot_eps), float(trans_eps))
    assert o
    cache = {}

    def lin(T):
        k = T.tobytes()
        if k not in cache:
            if len(cache) == 2:      # (the linearisation point and the last trial are all a pass can ask for)
                del cache[next(iter(cache))]
            cache[k] = linearize(src, dst, T, C_A, C_B, max_dist)
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
            if kind.value == 1:      # an LM trial: the error at Te on the correspondences of the linearisation at Tl, then the linearisation at Te
                at = lin(Tl)
                sums[28] = error(src, dst, Te, at["corr"], at["M"])
            r = lin(Te)
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
