"""VGICP's per-point covariances and one linearisation, restated in plain numpy: the reference the covariance kernels (csrc/cov_search.hip,
csrc/vgicp.hip: vgicp_cov_kernel, csrc/cov_math.h) and the voxel fold (vgicp_voxel_kernel) are checked against.  It shares nothing with
oracle/vgicp_oracle.c or the kernels: no k-d tree, no grid, no Jacobi sweeps, no "sort the three eigenvalues".

covariances(): for every query point
- neighbours by brute force over the cloud, float32 squared distances in fitness_ref.sq_dist_f32's expression (FLANN's L2_Simple<float>,
  fast_gicp_impl.hpp:250-253), ordered by (distance, original index) -- the rule tests/test_vgicp_gpu.py::test_neighbour_lists_* pin;
- the k neighbours as np.longdouble: mean over k, centred scatter over k, rounded to float64 (fast_gicp_impl.hpp:255-262);
- np.linalg.eigh, n = the eigenvector of the smallest eigenvalue, covariance = I - (1 - 1e-3) n n^T.  That is "singular values replaced by
  (1, 1, 1e-3)" (fast_gicp_impl.hpp:279-292) whenever the smallest eigenvalue is separated, whatever the order or rotation of the other two.

The error measure is err * gap: err the largest absolute entry difference of the 3x3 matrix, gap = (w1 - w0) / w2 of the scatter's eigenvalues
w0 <= w1 <= w2.  The eigenvector's sensitivity to a perturbation of the scatter is 1 / gap, so err * gap is free of the conditioning.
A query is `ambiguous` when its k-th and (k+1)-th float distances are unequal but within one float ulp of each other: another legitimate
evaluation order of the float expression could then change the list.  Exactly equal distances are not ambiguous: the index decides.

Clouds with fewer than k points are out of scope (the reference leaves those columns uninitialised).
"""
import collections

import numpy as np

import fitness_ref

K = 20

# Largest err * gap of oracle/vgicp_oracle.c (cyclic Jacobi, f64, mean about the origin) against covariances() over clouds() -- measured by
# tests/test_cov_ref.py::test_oracle_against_the_reference, which holds the oracle to twice this figure.  Per cloud (no query ambiguous, smallest
# gap 7.7e-4): lattice 6.6e-16, plane 2.1e-16, tilted 1.32e-15, line 2.1e-17, far_plane 9.3e-16, blob 8.0e-16, lidar 1.05e-15, two_planes 9.4e-16,
# clump 6.7e-16
ORACLE_ERR_GAP_MAX = 1.4e-15
# The device runs the oracle's algorithm with its own divide and square root and nothing else different: ten times the oracle's own error.
DEVICE_ERR_GAP_BOUND = 10 * ORACLE_ERR_GAP_MAX
# below this gap the smallest eigenvalue is not separated in float64 and the matrix is not defined by its neighbours
GAP_FLOOR = 1e-9

# The same for one linearisation over fold_map() / fold_scan() at resolutions 1.0, 0.5 and 2.0 and two poses: lin_diff() of the oracle on its own
# covariances against linearize() on covariances()'s, measured by tests/test_cov_ref.py::test_oracle_linearisation_against_the_transcription:
# H 1.27e-13, b 4.04e-13, err 1.09e-14 (the covariances of the worst-conditioned points differ by 4e-14).  The device gets ten times that.
ORACLE_LIN_MAX = (1.3e-13, 4.1e-13, 1.1e-14)
DEVICE_LIN_BOUND = tuple(10 * x for x in ORACLE_LIN_MAX)

CovRef = collections.namedtuple("CovRef", "cov gap ambiguous idx d2")


def _xyz32(cloud):
    a = np.asarray(cloud, np.float32)
    return np.ascontiguousarray(a.reshape(a.shape[0], -1)[:, :3])


def neighbours(pts, queries=None, k=K, chunk=64):
    """-> (idx (m, k) int64 in (distance, index) order, d2 (m, k + 1) float32: the k + 1 smallest distances, inf where the cloud ends)"""
    P = _xyz32(pts)
    q_rows = np.arange(P.shape[0]) if queries is None else np.asarray(queries, np.int64)
    n, kk = P.shape[0], min(k + 1, P.shape[0])
    assert n >= k, "clouds with fewer than k points are out of scope"
    idx = np.zeros((len(q_rows), k), np.int64)
    d2 = np.full((len(q_rows), k + 1), np.inf, np.float32)
    cols = np.asfortranarray(P)      # (each coordinate contiguous: the same numbers, read faster)
    for s in range(0, len(q_rows), chunk):
        d = fitness_ref.sq_dist_f32(P[q_rows[s:s + chunk]], cols)
        # the candidates: everything up to the (k + 1)-th smallest distance, ties included; then ordered by (distance, index)
        kth = np.partition(d, kk - 1, axis=1)[:, kk - 1]
        r, c = np.nonzero(d <= kth[:, None])
        dv = d[r, c]
        o = np.lexsort((c, dv, r))
        r, c, dv = r[o], c[o], dv[o]
        take = np.searchsorted(r, np.arange(d.shape[0]))[:, None] + np.arange(kk)[None, :]
        idx[s:s + chunk, :min(k, kk)] = c[take][:, :k]
        d2[s:s + chunk, :kk] = dv[take]
    return idx, d2


def covariances(pts, queries=None, k=K):
    """-> CovRef(cov (m, 3, 3) float64, gap (m,), ambiguous (m,) bool, idx (m, k), d2 (m, k + 1)); queries: rows of pts (default: all)"""
    P = _xyz32(pts)
    idx, d2 = neighbours(P, queries, k)
    nb = P[idx].astype(np.longdouble)                               # (m, k, 3)
    c = nb - (nb.sum(axis=1) / np.longdouble(k))[:, None, :]
    S = ((c[:, :, :, None] * c[:, :, None, :]).sum(axis=1) / np.longdouble(k)).astype(np.float64)
    w, V = np.linalg.eigh(S)
    nrm = V[:, :, 0]
    cov = np.eye(3)[None] - (1.0 - 1e-3) * nrm[:, :, None] * nrm[:, None, :]
    with np.errstate(all="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        a, b = d2[:, k - 1], d2[:, k]
        ambiguous = (a != b) & (b <= np.nextafter(a, np.float32(np.inf)))
    return CovRef(cov, gap, ambiguous, idx, d2)


def err_gap(got, ref):
    """per query: max |got - ref.cov| * ref.gap"""
    return np.abs(np.asarray(got) - ref.cov).max(axis=(1, 2)) * ref.gap


def eigenvalue_error(cov):
    """largest distance of any matrix's eigenvalues from (1e-3, 1, 1), and its largest asymmetry"""
    cov = np.asarray(cov)
    ev = np.linalg.eigvalsh(cov)
    return float(np.abs(ev - np.array([1e-3, 1.0, 1.0])).max()), float(np.abs(cov - cov.transpose(0, 2, 1)).max())


# ---------------------------------------------------------------------------
# the shared clouds: seeded, float32, 16-byte points, at most 6 m across unless said otherwise
# ---------------------------------------------------------------------------
def _cloud(xyz):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def lattice_slab(seed=31):
    """(a) 1/8 m lattice, three layers, 40 points duplicated: exact distance ties at the edge of most lists"""
    rng = np.random.default_rng(seed)
    p = np.zeros((2500, 3))
    p[:, :2] = rng.integers(-20, 20, (2500, 2)) / 8.0
    p[:, 2] = rng.integers(0, 3, 2500) / 8.0
    p[100:140] = p[200:240]
    return _cloud(p)


def plane_lattice(side=48):
    """(b) every site of a 0.25 m lattice at constant z (side 48: 11.75 m across; 24 for a cluster of a map): singular scatter"""
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return _cloud(np.stack([(i.ravel() - side // 2) * 0.25, (j.ravel() - side // 2) * 0.25, np.full(side * side, 0.75)], 1))


def tilted_plane(seed=33):
    """(c) z = 0.3 x - 0.2 y + 100 exactly: x and y on a 5/64 m lattice make every coordinate a float"""
    rng = np.random.default_rng(seed)
    site = rng.choice(72 * 72, 2500, replace=False)
    i, j = site // 72 - 36, site % 72 - 36
    return _cloud(np.stack([i * 5 / 64, j * 5 / 64, i * 3 / 128 - j / 64 + 100.0], 1))


def near_line(seed=34):
    """(d) y = x / 2, z noise 1e-3: two small eigenvalues"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.5, 2.5, 2500).astype(np.float32)
    return _cloud(np.stack([x, x / np.float32(2), rng.normal(0, 1e-3, 2500)], 1))


def far_plane(seed=35):
    """(e) a 2 cm thick plane centred at (1000, -2000, 30): the mean and the squares far from the origin"""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-2.5, 2.5, (2500, 2)), rng.uniform(-0.01, 0.01, (2500, 1))], 1)
    return _cloud(p + np.array([1000.0, -2000.0, 30.0]))


def blob(seed=36, n=2500):
    """(f) isotropic"""
    rng = np.random.default_rng(seed)
    return _cloud(np.clip(rng.normal(0, 0.8, (n, 3)), -3, 3))


_lidar = {}


def lidar_scan():
    """the lidar scan of tests/test_vgicp_gpu.py's vg_world"""
    if "scan" not in _lidar:
        from simpleslam_amd import synth
        world, _ = synth.make_map(60_000, seed=21)
        _lidar["scan"] = synth.make_scan(world, 0, seed=21, beams=32, azimuths=512)[0]
    return _lidar["scan"]


def lidar_cut():
    """(g) its first 3 000 points (tens of metres across)"""
    return np.ascontiguousarray(lidar_scan()[:3000])


def lidar_piece(k):
    """the scan's points within 2 m of its point 500 k in x and y, moved to the origin: a cluster of a map"""
    s = lidar_scan()
    c = s[500 * k, :3]
    p = s[(np.abs(s[:, :2] - c[:2]) <= 2.0).all(1) & (np.abs(s[:, 2] - c[2]) <= 3.0)].copy()
    p[:, :3] -= np.round(c)
    return p


def two_planes(seed=38):
    """(h) two exact planes 5 cm apart: the smallest eigenvalue tiny and not zero"""
    rng = np.random.default_rng(seed)
    return _cloud(np.concatenate([rng.integers(-160, 160, (2500, 2)) / 64.0, rng.choice(np.float32([0.0, 0.05]), (2500, 1))], 1))


def clump(seed=39):
    """(i) 3 000 points within 0.3 m: thousands of candidates per query"""
    rng = np.random.default_rng(seed)
    return _cloud(np.clip(rng.normal(0, 0.05, (3000, 3)), -0.15, 0.15))


_clouds = {}


def clouds():
    """name -> cloud, built once; treat as read-only"""
    if not _clouds:
        for name, make in (("lattice", lattice_slab), ("plane", plane_lattice), ("tilted", tilted_plane), ("line", near_line),
                           ("far_plane", far_plane), ("blob", blob), ("lidar", lidar_cut), ("two_planes", two_planes), ("clump", clump)):
            c = make()
            c.setflags(write=False)
            _clouds[name] = c
    return _clouds


_refs = {}


def reference(name):
    """covariances(clouds()[name]), computed once"""
    if name not in _refs:
        _refs[name] = covariances(clouds()[name])
    return _refs[name]


# ---------------------------------------------------------------------------
# one map-sized cloud of separated clusters
# ---------------------------------------------------------------------------
MAP_PITCH, MAP_SIDE, MAP_CLUSTER = 8.0, 10, 6.0
MAP_ORIGIN = np.array([960.0, -2040.0, 30.0])      # cluster (r, c) is centred at MAP_ORIGIN + (8 r, 8 c, 0): kilometres out, every offset a float


def cluster_map(n_min=300_001):
    """-> (cloud (n, 4) float32 with n just over n_min, clusters: list of (kind, first row, last row + 1)).  Cluster q of the 10 x 10 grid is one of
    the clouds above, centred and moved by integers; blobs of the size that makes up the count fill the grid."""
    kinds = ["lattice", "plane", "tilted", "line", "far_plane", "blob", "two_planes", "clump"] + [f"lidar{k}" for k in range(1, 13)]
    parts = []
    for kind in kinds:
        if kind.startswith("lidar"):
            p = lidar_piece(int(kind[5:]))
        elif kind == "plane":
            p = plane_lattice(24)
        else:
            p = clouds()[kind].copy()
        p = p.astype(np.float64)
        if kind in ("tilted", "far_plane"):
            p[:, :3] -= {"tilted": np.array([0.0, 0.0, 70.0]), "far_plane": np.array([1000.0, -2000.0, 0.0])}[kind]
        else:
            p[:, 2] += 30.0
        parts.append((kind, p))
    have = sum(len(p) for _, p in parts)
    n_fill = MAP_SIDE * MAP_SIDE - len(parts)
    per = -(-(n_min - have) // n_fill)
    for f in range(n_fill):
        p = blob(seed=1000 + f, n=per).astype(np.float64)
        p[:, 2] += 30.0
        parts.append(("blob", p))
    out, clusters, row = [], [], 0
    for q, (kind, p) in enumerate(parts):
        off = np.array([MAP_ORIGIN[0] + MAP_PITCH * (q // MAP_SIDE), MAP_ORIGIN[1] + MAP_PITCH * (q % MAP_SIDE), 0.0])
        assert (np.abs(p[:, :2]).max(0) <= MAP_CLUSTER / 2).all(), kind
        p[:, :3] += off
        out.append(p.astype(np.float32))
        clusters.append((kind, row, row + len(p)))
        row += len(p)
    return np.ascontiguousarray(np.concatenate(out)), clusters


def distance_to_other_clusters(pts, q):
    """lower bound of the distance from each point of cluster q to any point of another cluster: to the nearest face of its own 8 m cell in
    x and y, less the half-width other clusters may reach beyond theirs ((8 - 6) / 2 = 1 m short of the face)"""
    c = MAP_ORIGIN[:2] + MAP_PITCH * np.array([q // MAP_SIDE, q % MAP_SIDE])
    to_face = MAP_PITCH / 2 - np.abs(np.asarray(pts, np.float64)[:, :2] - c).max(axis=1)
    return to_face + (MAP_PITCH - MAP_CLUSTER) / 2


# ---------------------------------------------------------------------------
# one VGICP linearisation: a direct transcription of fast_vgicp_voxel.hpp:105-174 (ADDITIVE voxels) and fast_vgicp_impl.hpp:73-180
# ---------------------------------------------------------------------------
def voxel_coords(xyz, res):
    return np.floor(np.asarray(xyz, np.float64) / res - 0.5).astype(int)


def linearize(scan, m, pose, src_cov, dst_cov, res=1.0):
    """-> dict(H, b, err, n) in float64; src_cov / dst_cov: (n, 3, 3) covariances of the scan's and the map's points"""
    scan, m = np.asarray(scan), np.asarray(m)
    vox = {}
    for i, c in enumerate(map(tuple, voxel_coords(m[:, :3], res))):
        vox.setdefault(c, []).append(i)
    H, b, err, nc = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    R, t = pose[:3, :3], pose[:3, 3]
    for i in range(scan.shape[0]):
        tp = R @ scan[i, :3].astype(np.float64) + t
        c = tuple(np.floor(tp / res - 0.5).astype(int))
        if c not in vox:
            continue
        ids = vox[c]
        mean, CB = m[ids, :3].astype(np.float64).mean(0), dst_cov[ids].mean(0)
        M = np.linalg.inv(CB + R @ src_cov[i] @ R.T)
        e = mean - tp
        w = np.sqrt(len(ids))
        S = np.array([[0, -tp[2], tp[1]], [tp[2], 0, -tp[0]], [-tp[1], tp[0], 0]])
        J = np.concatenate([S, -np.eye(3)], 1)
        H += w * J.T @ M @ J; b += w * J.T @ M @ e; err += w * e @ M @ e; nc += 1
    return dict(H=H, b=b, err=float(err), n=nc)


def lin_diff(got, ref):
    """(dH, db, derr): largest entry difference of H and of b over the largest entry of the reference's, relative difference of the error"""
    return (float(np.abs(got["H"] - ref["H"]).max() / np.abs(ref["H"]).max()), float(np.abs(got["b"] - ref["b"]).max() / np.abs(ref["b"]).max()),
            float(abs(got["err"] - ref["err"]) / abs(ref["err"])))


# ---------------------------------------------------------------------------
# targets and scans for the voxel fold (vgicp_voxel_kernel): voxel c holds [(c + 0.5) res, (c + 1.5) res) on every axis
# ---------------------------------------------------------------------------
def fold_map(seed=51):
    """Voxels of 1, 2 and about 25 points and three of 400, 900 and 1 000 points at resolution 1.0; 700 of the last lie in one voxel of resolution
    0.5; 200 points in one voxel of resolution 2.0."""
    rng = np.random.default_rng(seed)
    box = lambda lo, size, n: np.asarray(lo, np.float64) + rng.uniform(0.02, 0.98, (n, 3)) * size
    parts = [box((0.5, 0.5, 0.5), 1.0, 400), box((2.5, 0.5, 0.5), 1.0, 900),
             box((0.75, 2.75, 0.75), 0.5, 700), box((0.5, 2.5, 0.5), 1.0, 300),       # [0.75, 1.25) is one voxel at 0.5 and inside one at 1.0
             box((7.0, 7.0, 1.0), 2.0, 200)]                                            # one voxel at 2.0, eight at 1.0
    for k in range(30):                                                                 # one point a voxel
        parts.append(box((12.5 + 2 * (k % 6), 0.5 + 2 * (k // 6), 0.5), 1.0, 1))
    for k in range(20):                                                                 # two
        parts.append(box((0.5 + 2 * (k % 5), 12.5 + 2 * (k // 5), 0.5), 1.0, 2))
    return _cloud(np.concatenate(parts))


def fold_scan(m, seed=52):
    """300 points near points of the map, and points exactly on voxel faces of resolutions 0.5, 1.0 and 2.0 (x / res - 0.5 an integer)"""
    rng = np.random.default_rng(seed)
    p = m[rng.choice(len(m), 300, replace=False), :3].astype(np.float64) + rng.normal(0, 0.01, (300, 3))
    faces = np.array([[0.5, 1.0, 1.0], [1.5, 1.0, 1.0], [1.0, 0.5, 1.5], [2.5, 1.5, 0.5], [3.5, 1.0, 1.0], [0.75, 2.75, 0.75], [1.25, 3.0, 1.0],
                      [1.0, 3.25, 1.25], [0.5, 2.5, 0.5], [1.5, 3.5, 1.5], [7.0, 8.0, 2.0], [9.0, 8.0, 2.0], [8.0, 7.0, 1.0], [8.0, 9.0, 3.0],
                      [8.5, 8.5, 1.5], [7.5, 7.5, 2.5], [3.0, 1.0, 1.0], [1.0, 1.0, 1.0], [8.0, 8.0, 2.0], [2.5, 0.5, 0.5]])
    return _cloud(np.concatenate([p, faces]))


def voxel_counts(m, res):
    _, cnt = np.unique(voxel_coords(np.asarray(m)[:, :3], res), axis=0, return_counts=True)
    return cnt


def fold_poses():
    """the identity (a scan point on a voxel face stays there) and a pose 5 cm and half a degree off"""
    from simpleslam_amd import synth
    return [np.eye(4), synth.perturb(np.eye(4), 7, trans=0.05, rot_deg=0.5)]
