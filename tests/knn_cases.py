"""Seeded inputs for the edge tests of pcr_knn and pcr_radius_search (tests/test_knn_query_edges_gpu.py): plain numpy, no GPU.  Each
generator returns a Case: the target, the queries and the k or radius values they are meant for.  tests/test_knn_cases.py holds every
input to the condition it was made for (ties that straddle the k-th place, points within two ulps of a cell face, segment lengths
around 64, 256 and 1024, counts on both sides of the scan's chunk seams), with tests/knn_ref.py alone.

The index of a point is its row in the target, as pcr_knn reports it.  The grid index stores a target by cell (z, then y, then x):
`storage` is a point's rank in that order, which the generators decouple from the row by a seeded permutation."""
from types import SimpleNamespace

import numpy as np

import knn_ref
import voxel_ref


def Case(target, queries, values, **more):
    return SimpleNamespace(target=target, queries=queries, values=values, **more)


def _cloud(xyz):
    c = np.zeros((len(xyz), 4), np.float32)
    c[:, :3] = xyz
    return c


def random_cloud(n=4000, seed=0, lo=(-10.0, -10.0, -3.0), hi=(10.0, 10.0, 3.0)):
    """n points uniform in a box of 20 x 20 x 6 m: 2 400 cells of 1 m, not quite two points a cell"""
    rng = np.random.default_rng(seed)
    return _cloud(rng.uniform(lo, hi, (n, 3)))


def random_queries(n, target, seed=0, spread=0.3):
    """n queries next to target points drawn at random"""
    rng = np.random.default_rng(seed)
    q = target[rng.integers(0, len(target), n)].copy()
    q[:, :3] += rng.normal(0, spread, (n, 3)).astype(np.float32)
    q[:, 3] = 0
    return q


# ---------------------------------------------------------------------------------------------------------------------------
# lattices: exact ties
# ---------------------------------------------------------------------------------------------------------------------------
TIE_KS = (1, 6, 7, 8, 16, 27, 32)


def lattice(shape=(12, 12, 6), pitch=1.0, origin=(0.0, 0.0, 0.0), copies=1, seed=0):
    """Every site of an integer lattice times `pitch`, plus `origin`, each `copies` times, the rows permuted.  pitch and origin must be
    short binary fractions: then every coordinate and every difference is exact in float32 and equal distances are equal in bits."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")      # x fastest: the index's cell order
    sites = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    xyz = np.repeat(sites * float(pitch) + np.asarray(origin, np.float64), copies, axis=0)
    assert (xyz.astype(np.float32).astype(np.float64) == xyz).all(), "pitch and origin must be exact in float32"
    perm = rng.permutation(len(xyz))
    target = _cloud(xyz[perm])
    storage = perm.copy()      # row r holds the point of lattice-order position perm[r]
    case = Case(target, None, TIE_KS, shape=tuple(shape), pitch=float(pitch), origin=tuple(float(o) for o in origin), copies=copies, storage=storage, seed=seed)
    case.queries = tie_queries(case)
    return case


def tie_queries(lat):
    """Queries at equal distances from many sites.  In units of the pitch, for an interior query: a site has 6 sites at d2 = 1, 12 at 2
    and 8 at 3; a cell centre 8 at 0.75 and 24 at 2.75; a face centre 4 at 0.5 and 8 at 1.5; an edge midpoint 2 at 0.25 and 8 at
    1.25.  Sites: all 8 corners, boundary and interior ones.  And sites one pitch outside the box, beyond faces, edges and corners."""
    rng = np.random.default_rng(lat.seed + 1000)
    n = np.asarray(lat.shape)

    def pick(m, lo, hi):      # m random integer triples, lo <= . < hi per axis
        return rng.integers(lo, hi, (m, 3)).astype(np.float64)

    corners = np.array([[i, j, k] for i in (0, n[0] - 1) for j in (0, n[1] - 1) for k in (0, n[2] - 1)], np.float64)
    boundary = pick(16, 0, n)
    boundary[np.arange(16), rng.integers(0, 3, 16)] = 0
    boundary[8:] = np.where(boundary[8:] == 0, (n - 1)[None, :], boundary[8:])
    interior = pick(32, 1, n - 1)
    centres = pick(48, -1, n) + 0.5      # cell centres, the layer of cells just outside the box included
    faces = pick(48, 0, n - 1)
    faces += 0.5
    faces[np.arange(48), rng.integers(0, 3, 48)] -= 0.5      # two half-steps: the centre of a face
    edges = pick(48, 0, n - 1)
    edges[np.arange(48), rng.integers(0, 3, 48)] += 0.5      # one half-step: the midpoint of an edge
    outside = pick(24, 0, n)
    for r in range(24):      # one, two or three coordinates one pitch outside
        for ax in rng.permutation(3)[:1 + r % 3]:
            outside[r, ax] = -1.0 if rng.random() < 0.5 else float(n[ax])
    sites = np.concatenate([corners, boundary, interior, centres, faces, edges, outside])
    xyz = sites * lat.pitch + np.asarray(lat.origin)
    assert (xyz.astype(np.float32).astype(np.float64) == xyz).all()
    return _cloud(xyz)


def lattices(copies):
    """The three lattices of the tie tests: every point on a face of a 1 m cell; half the pitch (every point on a face of the lattice
    shifted by half a cell as well); an origin that is no multiple of the cell"""
    return [lattice(pitch=1.0, origin=(0.0, 0.0, 0.0), copies=copies, seed=11),
            lattice(pitch=0.5, origin=(-3.0, 2.0, 0.0), copies=copies, seed=12),
            lattice(pitch=1.0, origin=(0.25, -0.375, 0.125), copies=copies, seed=13)]


# ---------------------------------------------------------------------------------------------------------------------------
# cell faces
# ---------------------------------------------------------------------------------------------------------------------------
FACE_KS = (1, 5, 20)
NEAR, FAR = (3.0, -2.0, 1.0), (270.0, -285.0, 255.0)


def face_cloud(cell, shift, centre, seed=0, float_lattice=False, half=3, reps=10, n_inside=1500, q_reps=4, q_inside=120):
    """Target points and queries on the faces (j + shift) cell of the 2 half cells around `centre`, per axis: the float32 nearest the face
    (voxel_ref.face_values) and one and two ulps on either side of it, the other two coordinates random in the block; some with all three
    coordinates on faces; and points inside the cells, so that the k-th neighbour often lies across a face.
    float_lattice: the handle computes the cell index in float (NDT): probes of the search's slop are added (_add_slop_probes).
    values: (FACE_KS, the radii of half a cell and of 1.5 cells)."""
    rng = np.random.default_rng(seed)
    cell = float(cell)
    c0 = np.floor(np.asarray(centre, np.float64) / cell - shift)
    lo, hi = (c0 - half + shift) * cell, (c0 + half + shift) * cell

    def make(per_face, inside):
        out = []
        for ax in range(3):
            v = voxel_ref.face_values(cell, c0[ax] + shift + np.arange(-half, half + 1))      # 5 values per face
            p = rng.uniform(lo, hi, (len(v) * per_face, 3))
            p[:, ax] = np.tile(v, per_face)
            out.append(p)
        v3 = [voxel_ref.face_values(cell, c0[ax] + shift + np.arange(-half + 1, half)) for ax in range(3)]
        out.append(np.stack([rng.choice(v3[ax], 15 * per_face) for ax in range(3)], axis=1))
        out.append(rng.uniform(lo, hi, (inside, 3)))
        p = _cloud(np.concatenate(out))
        return p[rng.permutation(len(p))]

    target, queries = make(reps, n_inside), make(q_reps, q_inside)
    case = Case(target, queries, (FACE_KS, (0.5 * cell, 1.5 * cell)), cell=cell, shift=float(shift), centre=tuple(centre), slop_probes=[])
    if float_lattice:
        _add_slop_probes(case, c0, half, lo, hi, rng)
    return case


def float_cell(x, cell):
    """floor(float32(x) * float32(1 / leaf)): the cell pcl::VoxelGrid's float arithmetic puts a coordinate into"""
    return np.floor(np.asarray(x, np.float32) * (np.float32(1.0) / np.float32(cell))).astype(np.float64)


def _add_slop_probes(case, c0, half, lo, hi, rng, per_value=6, d0=0.05):
    """For a lattice whose cell index is computed in float.  A face value v that float puts one cell higher than f64 does lies BELOW the
    lower face of the cell that holds it, by a fraction of an ulp: the margin that knn_query.hip's slop is there for.  Per such v, on
    every axis, a group of `per_value` probes: a point p at v, the query q straight below it by d = n ulps (about 5 cm), a decoy straight
    below q by the same d, later in the target than p.
    - k = 1 (the y and z axes, whose slab distances skip rows): the decoy's row is scanned first, p's slab then looks farther than d by
      the margin, and only the slop keeps its row from being skipped; at the tie the answer is p, the lower row.
    - radius search at the group's own radius, half-way between d and the distance to p's slab: p is inside it, q + r short of the slab.
    Appended after the permutation.  case.slop_probes = [group]: ax, qrows, prows, drows, d, gap, radius."""
    cell = case.cell
    P, D, Q = [], [], []
    n_t, n_q = len(case.target), len(case.queries)
    for ax in range(3):
        v = voxel_ref.face_values(cell, c0[ax] + np.arange(-half + 1, half))
        v = v[float_cell(v, cell) > np.floor(v.astype(np.float64) / cell)]
        for pv in v:
            step = np.spacing(np.float32(max(abs(pv), abs(pv - 1.0))))
            n = np.float32(round(d0 / float(step)))
            qa, da = np.float32(pv - n * step), np.float32(pv - 2 * n * step)
            d, gap = float(pv) - float(qa), float(float_cell(pv, cell)) * cell - float(qa)
            if not (0 < d == float(qa) - float(da) < gap):
                continue
            rows = []
            for _ in range(per_value):
                p = rng.uniform(lo, hi).astype(np.float32)
                q, dec = p.copy(), p.copy()
                p[ax], q[ax], dec[ax] = pv, qa, da
                rows.append(len(P))
                P.append(p); D.append(dec); Q.append(q)
            rows = np.array(rows)
            case.slop_probes.append(SimpleNamespace(ax=ax, qrows=n_q + rows, prows=n_t + rows, drows=None, d=d, gap=gap, radius=0.5 * (d + gap)))
    for g in case.slop_probes:
        g.drows = g.prows + len(P)      # the decoys after every p: the later row
    case.target = np.concatenate([case.target, _cloud(np.array(P + D))])
    case.queries = np.concatenate([case.queries, _cloud(np.array(Q))])


def ulps_from_a_face(x, cell, shift):
    """How many float32 steps x lies from the float32 nearest its nearest face (j + shift) cell: an int64 array"""
    x = np.asarray(x, np.float32)
    j = np.round(x.astype(np.float64) / cell - shift)
    f = ((j + shift) * cell).astype(np.float32)

    def order(a):      # float32 -> integers that step by one per ulp, monotone through zero
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(order(x) - order(f))


# ---------------------------------------------------------------------------------------------------------------------------
# shells: radius segments of a chosen length
# ---------------------------------------------------------------------------------------------------------------------------
SHELL_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)


def shells(n=2500, centre=(10.5, 20.5, 2.5), seed=0, step=1e-3):
    """n points at distances step, 2 step, ... n step from `centre` (a cell centre).  n step = 2.5 m does not fit into one 1 m cell, so the
    directions are random within the row of cells through `centre` along x (|dy|, |dz| < 0.4): one row of the index holds all n, its
    centre cell the first few hundred, far more than 64 either way.  A thin background lies beyond the last shell.
    radius(m): half-way between the m-th and the (m + 1)-th of the f64 distances knn_ref computes from `centre` (never from the
    construction), so that a query at `centre` has exactly m hits.  queries: the centre, a point with no hit at any of the radii, the
    centre again."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    d = step * np.arange(1, n + 1)
    w = np.minimum(0.4, d / 2)
    dy, dz = rng.uniform(-w, w), rng.uniform(-w, w)
    dx = np.sqrt(d * d - dy * dy - dz * dz) * rng.choice([-1.0, 1.0], n)
    pts = c + np.stack([dx, dy, dz], axis=1)
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    back = c + u * rng.uniform(n * step + 0.5, n * step + 6.0, (200, 1))
    target = _cloud(np.concatenate([pts, back]))
    target = target[rng.permutation(len(target))]
    queries = _cloud(np.array([c, c + [0.0, 300.0, 0.0], c]))
    _, d2 = knn_ref.knn(target, queries[:1], len(target))
    dist = np.sqrt(d2[0])

    def radius(m):
        return float(0.5 * dist[0]) if m == 0 else float(0.5 * (dist[m - 1] + dist[m]))
    return Case(target, queries, SHELL_LENGTHS, radius=radius, dist=dist, centre=tuple(centre))


# ---------------------------------------------------------------------------------------------------------------------------
# mixed queries: counts on both sides of the scan's chunk seams
# ---------------------------------------------------------------------------------------------------------------------------
MIXED_RADIUS = 1.5
MIXED_SIZES = (1, 1023, 1024, 1025, 2049, 3100)
IN, OUT, BAD, COPY = 0, 1, 2, 3
_SEAM = (IN, OUT, BAD, IN, OUT, COPY, IN, OUT)      # the kinds at positions s - 4 .. s + 3 of a seam s


def mixed_queries(n, target, seed=0):
    """n queries: about a third next to target points, about a third 100 m and more outside the cloud (no hit at MIXED_RADIUS), the rest
    with a coordinate that is not finite or exact copies of target points.  Around the positions 1024 and 2048, where radius_scan_kernel
    hands its carry on, the kinds are set so that queries with and without hits lie on both sides.  values: MIXED_RADIUS."""
    rng = np.random.default_rng(seed)
    kind = rng.choice([IN, OUT, BAD, COPY], n, p=[0.34, 0.33, 0.13, 0.20])
    for s in (1024, 2048):
        for o, kd in enumerate(_SEAM):
            if 0 <= s - 4 + o < n:
                kind[s - 4 + o] = kd
    q = target[rng.integers(0, len(target), n)].copy()
    q[:, 3] = 0
    lo, hi = target[:, :3].min(axis=0), target[:, :3].max(axis=0)
    for j in range(n):
        if kind[j] == IN:
            q[j, :3] += rng.normal(0, 0.3, 3).astype(np.float32)
        elif kind[j] == OUT:
            ax, far = rng.integers(0, 3), np.float32(rng.uniform(100.0, 400.0))
            q[j, ax] = hi[ax] + far if rng.random() < 0.5 else lo[ax] - far
        elif kind[j] == BAD:
            q[j, rng.integers(0, 3)] = rng.choice([np.nan, np.inf, -np.inf])
    return Case(target, q, MIXED_RADIUS, kind=kind)
