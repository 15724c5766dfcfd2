"""NDT voxel Gaussians (pclomp VoxelGridCovariance, voxel_grid_covariance_omp_impl.hpp:49-370) in plain Python/numpy: the exact reference
ndt_voxel_kernel and the oracle's ndt_grid_build are both held to (tests/test_ndt_voxel_ref.py, tests/test_ndt_voxels_gpu.py).  Shares no
code with either.

  membership   float32 floor(p * float32(1 / leaf)), as the reference builds its lattice (:218-220)
  mean, cov    exact: every float32 coordinate is an integer times 2^-149, the sums of x and x x^T are Python integers,
               mean = S1 / n and cov = (S2 / n - mean mean^T) (n - 1) / n are rationals, each rounded ONCE to double
  the rest     float64: numpy's eigh, eigenvalues below 0.01 * the largest raised to it (at most two, :345-356), the inverse, the
               inf test (:359-364)

lam_min / lam_max are the extreme eigenvalues of that once-rounded covariance (eigh: good to an ulp of lam_max), R the largest
|coordinate| among the voxel's points, raised how many eigenvalues the clamp moved.  `kept` is the reference's own verdict (:337-341 on
the exact covariance); mean and icov are filled in either way, so that a voxel whose verdict hangs on the rounding of an inexact
implementation can still be compared.
"""
import math

import numpy as np

_SHIFT = 149      # every finite float32 is an integer multiple of 2^-149


def _as_int(x):
    """float32 value -> the integer x * 2^149, exactly"""
    m, e = math.frexp(float(x))
    return int(m * 16777216.0) << (e - 24 + _SHIFT) if e - 24 + _SHIFT >= 0 else int(m * 16777216.0) >> -(e - 24 + _SHIFT)


def lattice(pts, leaf):
    """(finite mask, ijk of every finite point) by the build's rounding: float32 floor(p * float32(1 / leaf))"""
    p = np.asarray(pts, np.float32)[:, :3]
    ok = np.isfinite(p).all(axis=1)
    inv = np.float32(1.0) / np.float32(leaf)
    return ok, np.floor(p[ok] * inv).astype(np.int64)


def lattice_lookup(pts, leaf):
    """ijk by the LOOKUP's rounding: float32 floor(p / float32(leaf)) (:380-382)"""
    p = np.asarray(pts, np.float32)[:, :3]
    return np.floor(p / np.float32(leaf)).astype(np.int64)


def exact_voxels(pts, leaf, min_points=6, eig_mult=0.01):
    """Every voxel with at least max(3, min_points) points, sorted by (ix, iy, iz):
    dict(ijk (m,3), n, mean (m,3), cov (m,3,3) unclamped, icov (m,3,3), kept (m,) bool, raised (m,), lam_min, lam_max, lam_min_clamped, R)"""
    min_points = max(3, int(min_points))
    p = np.asarray(pts, np.float32)[:, :3]
    ok, ijk = lattice(p, leaf)
    p = p[ok]
    out = dict(ijk=[], n=[], mean=[], cov=[], icov=[], kept=[], raised=[], lam_min=[], lam_max=[], lam_min_clamped=[], R=[])
    if len(p):
        uniq, inv, counts = np.unique(ijk, axis=0, return_inverse=True, return_counts=True)
        order = np.argsort(inv.ravel(), kind="stable")
        starts = np.r_[0, np.cumsum(counts)]
        for v in range(len(uniq)):          # (np.unique sorts rows lexicographically: (ix, iy, iz))
            n = int(counts[v])
            if n < min_points:
                continue
            q = p[order[starts[v]:starts[v + 1]]]
            X = [[_as_int(c) for c in row] for row in q]
            S1 = [sum(r[k] for r in X) for k in range(3)]
            S2 = [[sum(r[a] * r[b] for r in X) for b in range(3)] for a in range(3)]
            mean = np.array([S1[k] / (n << _SHIFT) for k in range(3)])          # int / int: correctly rounded
            den = n ** 3 << (2 * _SHIFT)
            cov = np.array([[((n * S2[a][b] - S1[a] * S1[b]) * (n - 1)) / den for b in range(3)] for a in range(3)])
            w, V = np.linalg.eigh(cov)
            kept = not (w[0] < 0 or w[1] < 0 or w[2] <= 0)
            wc, raised = w.copy(), 0
            if w[2] > 0:
                minev = eig_mult * w[2]
                if wc[0] < minev:
                    wc[0] = minev; raised = 1
                    if wc[1] < minev:
                        wc[1] = minev; raised = 2
            c2 = (V * wc) @ V.T if raised else cov
            with np.errstate(all="ignore"):
                try:
                    icov = np.linalg.inv(c2)
                except np.linalg.LinAlgError:
                    icov = np.full((3, 3), np.inf)
            if not np.isfinite(icov).all():
                kept = False
            out["ijk"].append(uniq[v]); out["n"].append(n); out["mean"].append(mean); out["cov"].append(cov); out["icov"].append(icov)
            out["kept"].append(kept); out["raised"].append(raised); out["lam_min"].append(w[0]); out["lam_max"].append(w[2])
            out["lam_min_clamped"].append(wc[0]); out["R"].append(float(np.abs(q.astype(np.float64)).max()))
    shapes = dict(ijk=(0, 3), mean=(0, 3), cov=(0, 3, 3), icov=(0, 3, 3))
    res = {}
    for k, v in out.items():
        dt = np.int64 if k in ("ijk", "n", "raised") else (bool if k == "kept" else np.float64)
        res[k] = np.array(v, dt) if v else np.zeros(shapes.get(k, (0,)), dt)
    return res


# What an implementation that feeds (nearly) exact sums into the reference's cancelling single-pass expression (:329-330) may differ from
# the exact values by.  eps = 2^-53.
EPS = 2.0 ** -53
# mean = sum / n with an exact sum of at most n R: the sum is rounded once (half an ulp: eps * n R), the quotient once more (eps * R),
# and an implementation that carries the sum as n * centre + a centred part rounds that product too (eps * n R): 3 eps R in all; 4 asked.
MEAN_ULPS = 4.0
# The device's sums are exact only on its fixed-point grid (csrc/ndt.hip, ndt_voxel_kernel): every x - centre is rounded to a multiple of
# 2^-44 and every product (x - centre)(y - centre) to a multiple of 2^-40 before the integers are added up.
#   first moments   the leaf is a float32, so a centre (k + 0.5) * leaf is dyadic whatever the leaf (0.3f = m * 2^-25: centres are
#                   multiples of 2^-26), and a float32 coordinate of magnitude >= 2^-21 minus it is on the 2^-44 grid: the sum is exact
#                   and 4 eps R is the whole error of the mean, on every lattice.  No quantum enters the mean.
#   second moments  a product of two centred coordinates is on the 2^-40 grid when both are multiples of 2^-20 (coordinates of magnitude
#                   >= 8 m with leaves that are multiples of 2^-19, or a binary-lattice cloud); a voxel near the origin is not.  Up to
#                   2^-41 per term, hence per entry of the covariance, whatever n and R.
COV_QUANTUM = 2.0 ** -41


def mean_bound(ref):
    return MEAN_ULPS * EPS * ref["R"]


# The clamp rebuilds the covariance from its eigen-decomposition (:345-356).  Two backward-stable 3 x 3 solvers fed the SAME covariance
# each return V diag(w) V^-1 = cov + E with ||E|| of a few eps * lam_max; 8 eps lam_max is allowed per solver (a cyclic Jacobi of a
# handful of sweeps, three rotations each).  The inverse moves by icov (E1 - E2) icov: at most ||icov||_2 * 16 eps lam_max / lam_min
# with ||icov||_2 <= 3 ||icov||_max.  For a voxel whose sums are the oracle's bit for bit (re-summed in input order) this is the whole
# difference between the device's icov and the oracle's.
SOLVER_ULPS = 8.0


def icov_solver_bound(ref):
    nrm = np.abs(ref["icov"]).reshape(-1, 9).max(axis=1) if len(ref["n"]) else np.zeros(0)
    return 3.0 * 2.0 * SOLVER_ULPS * EPS * ref["lam_max"] / ref["lam_min_clamped"] * nrm


def icov_bound_unit(ref):
    """2^-53 * n * R^2 / lam_min(clamped) * ||icov||_max per voxel: the bound of the icov comparison is K times this.  n R^2 eps is the
    rounding of the sums of squares about the origin, which the expression's cancellation leaves standing in full beside a covariance of
    size lam; lam_min(clamped) is what the inverse divides by."""
    nrm = np.abs(ref["icov"]).reshape(-1, 9).max(axis=1) if len(ref["n"]) else np.zeros(0)
    return EPS * ref["n"] * ref["R"] ** 2 / ref["lam_min_clamped"] * nrm


def icov_quantum_bound(ref):
    """What the fixed-point grid adds to the device's icov error (it matters where n R^2 2^-53 is below 2^-40: voxels within ~20 m of the
    origin).  A perturbation D of the covariance moves its inverse by icov D icov to first order: at most ||icov||_2 ||D||_2 / lam_min,
    with ||D||_2 <= 3 COV_QUANTUM and ||icov||_2 <= 3 ||icov||_max for 3 x 3 matrices."""
    nrm = np.abs(ref["icov"]).reshape(-1, 9).max(axis=1) if len(ref["n"]) else np.zeros(0)
    return 9.0 * COV_QUANTUM / ref["lam_min_clamped"] * nrm


# K of the icov comparison.  The largest (oracle - exact) / icov_bound_unit over every case of tests/ndt_clouds.py:all_voxel_cases, measured
# on the CPU by tests/test_ndt_voxel_ref.py::test_oracle_error_sets_K, is 0.225 (generic cloud about the origin at 0.5 m; 0.07 .. 0.22 on
# the others).  The device gets a margin of 4 on top: its eigenvectors come from another eigen-solver and another libm.
ICOV_K_MEASURED = 0.225
ICOV_K = 4 * ICOV_K_MEASURED


def sort_xyz(v):
    """a dict of per-voxel arrays (with `ijk`) sorted by (ix, iy, iz), like exact_voxels' output"""
    o = np.lexsort((v["ijk"][:, 2], v["ijk"][:, 1], v["ijk"][:, 0]))
    return {k: (a[o] if isinstance(a, np.ndarray) and a.shape[:1] == (len(o),) else a) for k, a in v.items()}
