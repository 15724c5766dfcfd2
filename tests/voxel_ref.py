"""A plain numpy restatement of pcl::VoxelGrid<PointT>::applyFilter as the reference calls it (pcp.hpp:14-28, LidarOdometry.cpp:36):
leaf (g, g, g) as float, downsample_all_data on, no field limits, min_points_per_voxel 0.  Every step that PCL takes in float is taken
here in float32; the voxel index is formed in 64-bit integers, so it never overflows.

This is the exact reference the voxel-filter tests compare the oracle (oracle/voxel_oracle.c) and the device (pcr_voxel_filter) with:

  - the minimum and maximum over the finite points (getMinMax3D);
  - inv = 1.0f / leaf;
  - the too-fine test as PCL writes it (voxel_grid.hpp; the reference's own copy of it:
    third_parties/pclomp/src/voxel_grid_covariance_omp_impl.hpp:74-79):
        d = int64((max - min) * inv) + 1 per axis, in float;  dx * dy * dz > INT_MAX  ->  output = input, non-finite rows included;
  - min_b = floor(min * inv);  ijk = int(floor(p * inv) - float(min_b));  div_b = floor(max * inv) - min_b + 1;
  - idx = ijk0 + ijk1 * div_b0 + ijk2 * div_b0 * div_b1, voxels in ascending idx, i.e. in (z, y, x) order.

PCL forms idx in `int`.  Its too-fine test bounds (max - min) * inv, not the floor-based div_b, so a box just under its limit can still
have div_b0 * div_b1 * div_b2 > INT_MAX, and idx then wraps in PCL.  What PCL's output order is in that window cannot be observed
without PCL itself; this restatement keeps the ascending order of the true (64-bit) index there.
"""
import numpy as np

INT_MAX = 2**31 - 1


def _f32(pts):
    a = np.ascontiguousarray(pts, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("clouds must have shape (n, >= 3)")
    return a


def pcl_axis_counts(mn, mx, leaf):
    """PCL's voxel count per axis for the box [mn, mx] (float32 triples): int64((max - min) * inv) + 1, all in float."""
    inv = np.float32(1.0) / np.float32(leaf)
    span = (np.asarray(mx, np.float32) - np.asarray(mn, np.float32)) * inv          # float32 throughout
    out = []
    for v in span:
        v = float(v)
        out.append(int(v) + 1 if np.isfinite(v) else None)      # (an infinite span: no int64 holds it, the box is too fine by any count)
    return out


def floor_axis_counts(mn, mx, leaf):
    """The lattice's voxel count per axis, floor(max * inv) - floor(min * inv) + 1 (float products, exact integer difference)."""
    inv = np.float32(1.0) / np.float32(leaf)
    lo = np.floor(np.asarray(mn, np.float32) * inv)
    hi = np.floor(np.asarray(mx, np.float32) * inv)
    return [int(h) - int(l) + 1 for l, h in zip(lo, hi)]


def pcl_too_fine(mn, mx, leaf):
    """PCL's "Leaf size is too small for the input dataset" decision for the box [mn, mx]."""
    d = pcl_axis_counts(mn, mx, leaf)
    if any(v is None for v in d):
        return True
    return d[0] * d[1] * d[2] > INT_MAX


def intensity_column(stride):
    """The channel averaged besides xyz: data[4] of pcl::PointXYZI (stride 8), float 3 of a 16- to 28-byte point, none for 12 bytes."""
    return 4 if stride >= 8 else (3 if stride >= 4 else None)


class VoxelRef:
    """voxel_ref(pts, leaf) -> VoxelRef.

    unfiltered    PCL's too-fine path was taken: the output is the input
    finite        bool per point
    voxel         per point: its voxel index (int64), -1 for a non-finite point (or for every point when unfiltered)
    ids           per voxel, ascending: its index
    members(v)    the input rows of voxel v, in input order
    mean64        per voxel: the float64 mean of its members (all columns), rounded to float32, in PCL's output layout
    sum32         per voxel: float32 sums in input order divided by the float32 count -- what the oracle forms -- in PCL's layout
    min_b, div_b  the lattice (int64 triples), None when there is no finite point or when unfiltered
    """

    def __init__(self, pts, leaf):
        pts = _f32(pts)
        self.pts, self.leaf = pts, np.float32(leaf)
        n, stride = pts.shape
        self.stride = stride
        self.finite = np.isfinite(pts[:, :3]).all(1)
        self.voxel = np.full(n, -1, np.int64)
        self.unfiltered = False
        self.min_b = self.div_b = None
        self.ids = np.zeros(0, np.int64)
        self._order = np.zeros(0, np.int64)
        self._start = np.zeros(1, np.int64)
        if not self.finite.any():
            self.mean64 = self.sum32 = np.zeros((0, stride), np.float32)
            return
        fin = pts[self.finite, :3]
        mn, mx = fin.min(0), fin.max(0)
        self.box = (mn, mx)
        if pcl_too_fine(mn, mx, leaf):
            self.unfiltered = True
            self.mean64 = self.sum32 = pts.copy()
            return
        inv = np.float32(1.0) / np.float32(leaf)
        min_b = np.floor(mn * inv)                                                   # float32, integral
        max_b = np.floor(mx * inv)
        self.min_b = min_b.astype(np.int64)
        self.div_b = max_b.astype(np.int64) - self.min_b + 1
        ijk = (np.floor(fin * inv) - min_b.astype(np.float32)).astype(np.int64)     # float32 subtraction, as PCL's static_cast<float>(min_b)
        d0, d1 = int(self.div_b[0]), int(self.div_b[1])
        vid = ijk[:, 0] + ijk[:, 1] * d0 + ijk[:, 2] * (d0 * d1)                     # int64: never wraps
        self.voxel[self.finite] = vid
        rows = np.flatnonzero(self.finite)
        o = np.argsort(vid, kind="stable")                                           # input order inside a voxel
        self._order = rows[o]
        sv = vid[o]
        self.ids, start, cnt = np.unique(sv, return_index=True, return_counts=True)
        self._start = np.append(start, len(sv)).astype(np.int64)
        self.counts = cnt
        self.mean64 = self._layout(self._mean64(start, cnt))
        self.sum32 = self._layout(self._sum32(start, cnt))

    def __len__(self):
        return self.pts.shape[0] if self.unfiltered else len(self.ids)

    def members(self, v):
        return self._order[self._start[v]:self._start[v + 1]]

    def _values(self):
        """the channels that are averaged: x, y, z and the intensity column (if any)"""
        ic = intensity_column(self.stride)
        cols = [0, 1, 2] + ([ic] if ic is not None else [])
        return self.pts[self._order][:, cols], ic

    def _mean64(self, start, cnt):
        vals, ic = self._values()
        s = np.add.reduceat(vals.astype(np.float64), start, axis=0)
        return (s / cnt[:, None]).astype(np.float32), ic

    def _sum32(self, start, cnt):
        """float32 sums in input order (one voxel's additions strictly one after the other), divided by the float32 count"""
        vals, ic = self._values()
        rank = np.arange(len(vals)) - np.repeat(start, cnt)
        vox = np.repeat(np.arange(len(cnt)), cnt)
        acc = np.zeros((len(cnt), vals.shape[1]), np.float32)
        by_rank = np.argsort(rank, kind="stable")
        rk = rank[by_rank]
        edges = np.searchsorted(rk, np.arange(int(cnt.max()) + 1))
        for k in range(int(cnt.max())):                     # the k-th member of every voxel that has one: no voxel twice per step
            sel = by_rank[edges[k]:edges[k + 1]]
            acc[vox[sel]] += vals[sel]
        return acc / cnt.astype(np.float32)[:, None], ic

    def _layout(self, cv):
        c, ic = cv
        out = np.zeros((c.shape[0], self.stride), np.float32)
        out[:, :3] = c[:, :3]
        if self.stride >= 8:
            out[:, 3] = 1.0                                     # pcl::PointXYZI keeps data[3] = 1
        if ic is not None:
            out[:, ic] = c[:, 3]
        return out


def voxel_ref(pts, leaf):
    return VoxelRef(pts, leaf)


def ulp_distance(a, b):
    """|a - b| in float32 ulps, element-wise (both finite float32): the distance between their positions on the ordered float line."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def assert_matches_ref(got, ref, max_ulp=1, what=""):
    """The device's output against the reference: the same number of rows, every averaged channel within max_ulp float32 ulps of the
    float64 mean, the constant channels exact.  A point in the wrong voxel moves its centroid by far more than an ulp."""
    got = np.asarray(got, np.float32)
    assert got.shape == (len(ref), ref.stride), f"{what}: {got.shape} rows vs {len(ref)} in the reference"
    if ref.unfiltered:
        np.testing.assert_array_equal(got, ref.pts, err_msg=f"{what}: the unfiltered input")
        return
    d = ulp_distance(got, ref.mean64)
    if d.size and d.max() > max_ulp:
        r, c = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError(f"{what}: row {r} col {c}: {got[r, c]!r} vs mean {ref.mean64[r, c]!r} ({d[r, c]} ulps); "
                             f"{int((d > max_ulp).any(1).sum())} of {len(ref)} rows off")


# ---------------------------------------------------------------------------
# Adversarial inputs (seeded): where float and double arithmetic disagree about the voxel, far from the origin, awkward content
# ---------------------------------------------------------------------------
def face_values(leaf, ks, ulps=(-2, -1, 0, 1, 2)):
    """float(k * leaf) and the floats `ulps` steps away from it, for every k in ks (float32, one array)."""
    x = (np.asarray(ks, np.float64) * float(leaf)).astype(np.float32)
    out = []
    for u in ulps:
        y = x.copy()
        for _ in range(abs(u)):
            y = np.nextafter(y, np.float32(np.inf if u > 0 else -np.inf))
        out.append(y)
    return np.concatenate(out)


def disagrees(x, leaf):
    """floor(float(x) * inv_f) != floor(double(x) / double(leaf)): the float lattice and the exact one put x in different voxels."""
    x = np.asarray(x, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(x * inv).astype(np.float64) != np.floor(x.astype(np.float64) / float(leaf))


def face_cloud(leaf, sign=1.0, n=20000, k0=1, nk=40, seed=0, stride=4, only_disagreeing=True):
    """Points whose coordinates sit on the voxel faces k * leaf (k = k0 .. k0 + nk - 1, times sign) and 1-2 ulps either side -- only those
    on which float and double disagree, unless the leaf is exact (then none do) -- plus one point at the centre of every voxel they touch,
    so that a point put into the wrong voxel moves a centroid by a good fraction of the leaf.  Returns (cloud, face values used)."""
    rng = np.random.default_rng(seed)
    ks = sign * np.arange(k0, k0 + nk)
    v = face_values(leaf, ks)
    if only_disagreeing:
        v = v[disagrees(v, leaf)]
    c = np.zeros((n, stride), np.float32)
    c[:, :3] = rng.choice(v, size=(n, 3))
    inv = np.float32(1.0) / np.float32(leaf)
    cells = np.unique(np.floor(c[:, :3] * inv), axis=0)
    centre = ((cells.astype(np.float64) + 0.5) * float(leaf)).astype(np.float32)
    pts = np.zeros((n + len(centre), stride), np.float32)
    pts[:n] = c
    pts[n:, :3] = centre
    if stride > 3:
        pts[:, 3] = rng.random(len(pts), dtype=np.float32) * 100
    pts = pts[rng.permutation(len(pts))]
    return pts, v


def far_cloud(leaf, log2_ratio, sign=1.0, n=20000, span=40, seed=0, stride=4):
    """A cloud whose coordinates / leaf lie around sign * 2^log2_ratio (2^23 .. 2^25: a UTM-like map at a small leaf): voxel-face points
    (float(k * leaf) +- 2 ulps) mixed with random points in a box of `span` voxels."""
    rng = np.random.default_rng(seed)
    base = np.round(2.0 ** log2_ratio)
    ks = sign * (base + np.arange(span))
    v = face_values(leaf, ks)
    m = n // 2
    pts = np.zeros((n, stride), np.float32)
    pts[:m, :3] = rng.choice(v, size=(m, 3))
    lo = sign * base * float(leaf)
    pts[m:, :3] = (lo + sign * rng.random((n - m, 3)) * span * float(leaf)).astype(np.float32)
    if stride > 3:
        pts[:, 3] = rng.random(n, dtype=np.float32) * 100
    return pts


def awkward_clouds(seed=0, stride=4):
    """name -> cloud: duplicated points, a lattice-quantised cloud, NaN / +Inf / -Inf rows in each axis separately, and voxels of
    1, 63, 64, 65 and 100 000 points; every one with its leaf."""
    rng = np.random.default_rng(seed)
    out = {}
    base = np.zeros((3000, stride), np.float32)
    base[:, :3] = rng.random((3000, 3), dtype=np.float32) * 20 - 10
    if stride > 3:
        base[:, 3] = rng.random(3000, dtype=np.float32) * 100
    out["duplicates"] = (np.concatenate([base[:500]] * 7)[rng.permutation(3500)], 0.3)
    q = np.zeros((8000, stride), np.float32)
    q[:, :3] = (rng.integers(-40, 40, (8000, 3)) * 0.1).astype(np.float32)       # multiples of 0.1: every coordinate near a face
    if stride > 3:
        q[:, 3] = rng.random(8000, dtype=np.float32)
    out["lattice_0.1"] = (q, 0.1)
    out["lattice_0.2_on_0.1"] = (q, 0.2)
    for ax in range(3):
        for name, val in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            c = base.copy()
            c[rng.choice(3000, 97, replace=False), ax] = val
            out[f"{name}_axis{ax}"] = (c, 0.5)
    sizes = [1, 63, 64, 65, 100_000, 1, 2, 65, 63]
    chunks = []
    for k, m in enumerate(sizes):
        c = np.zeros((m, stride), np.float32)
        c[:, :3] = np.array([2.0 * k, -2.0 * (k % 3), 1.0 * k], np.float32) + 0.05 + 0.9 * rng.random((m, 3), dtype=np.float32)
        if stride > 3:
            c[:, 3] = rng.random(m, dtype=np.float32) * 100
        chunks.append(c)
    v = np.concatenate(chunks)
    out["voxel_sizes"] = (v[rng.permutation(len(v))], 1.0)
    return out


def _jitter(x, rng):
    """x moved by -2 .. +2 float32 ulps, element-wise"""
    x = x.copy()
    u = rng.integers(-2, 3, x.shape)
    for _ in range(2):
        x = np.where(u > 0, np.nextafter(x, np.float32(np.inf)), np.where(u < 0, np.nextafter(x, np.float32(-np.inf)), x))
        u = u - np.sign(u)
    return x


def near_limit_boxes(n_boxes, seed=0):
    """Seeded boxes (two points each: the minimum corner and the maximum) whose voxel count lies within a few voxels per axis of INT_MAX,
    corners on voxel faces or 1-2 ulps off them: -> list of (leaf, mn, mx), float32 triples.  Two axes take a few hundred to a few thousand
    voxels, the third is sized to land the product on INT_MAX, and its corners are picked among many candidates so that the boxes include
    (when the candidates allow it) ones where PCL's count and the floor count fall on opposite sides of INT_MAX, in both directions."""
    rng = np.random.default_rng(seed)
    leaves = [0.05, 0.1, 0.3, 0.25, 0.5, 0.07]
    out = []
    for i in range(n_boxes):
        leaf = leaves[i % len(leaves)]
        inv = np.float32(1.0) / np.float32(leaf)

        def axes(m, span):
            k = rng.integers(-3_000_000, 3_000_000, m)
            a = _jitter(((k + rng.choice([0.0, 0.5, 0.001, 0.999], m)) * leaf).astype(np.float32), rng)
            b = _jitter(((k + span + rng.choice([0.0, 0.5, 0.001, 0.999], m)) * leaf).astype(np.float32), rng)
            b = np.maximum(a, b)
            pcl = np.trunc((b - a) * inv).astype(np.int64) + 1
            flo = np.floor(b * inv).astype(np.int64) - np.floor(a * inv).astype(np.int64) + 1
            return a, b, pcl, flo

        want = i % 3                    # 0: any, 1: PCL too fine and the floor count not, 2: the other way round
        for _ in range(20):             # (1: two axes on which both counts agree, so that the third decides)
            a01, b01, p01, f01 = axes(2, rng.integers(300, 5000, 2))
            if want != 1 or np.array_equal(p01, f01):
                break
        d2 = int(INT_MAX // (p01[0] * p01[1])) + (int(rng.integers(-1, 2)) if want != 1 else 0)
        # (1: PCL's count exceeds the floor count on an axis for about one corner pair in 7 000: many candidates around the span that puts the
        #  floor count exactly on INT_MAX // (d0 * d1))
        cand = [axes(4096 if want != 1 else 16384, max(d2 - 1 + o, 0)) for o in ((0,) if want != 1 else (-1, 0))]
        a2, b2, p2, f2 = (np.concatenate([c[q] for c in cand]) for q in range(4))
        pp, pf = p01[0] * p01[1] * p2, f01[0] * f01[1] * f2
        pick = np.flatnonzero((pp > INT_MAX) & (pf <= INT_MAX) if want == 1 else (pf > INT_MAX) & (pp <= INT_MAX))
        j = int(rng.choice(pick)) if want and len(pick) else int(rng.integers(0, len(a2)))
        mn = np.array([a01[0], a01[1], a2[j]], np.float32)
        mx = np.array([b01[0], b01[1], b2[j]], np.float32)
        perm = rng.permutation(3)
        out.append((leaf, mn[perm], mx[perm]))
    return out


def cube_1290():
    """The box of x in [0.05, 129.0], y and z in [0, 128.95] at leaf 0.1: PCL counts 1290^3 = 2 146 689 000 voxels (<= INT_MAX, it filters),
    the lattice's floor count is 1291 * 1290^2 = 2 148 353 100 (> INT_MAX)."""
    return 0.1, np.array([0.05, 0.0, 0.0], np.float32), np.array([129.0, 128.95, 128.95], np.float32)
