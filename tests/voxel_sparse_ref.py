"""A plain numpy and dict restatement of the reference's own voxel filters, pcp::VoxelDownSampleV3 (common/pcp/pcp.hpp:157-263) and
pcp::VoxelDownSampleV2 (pcp.hpp:78-154), with the choices pcr_voxel_filter_sparse documents where the reference leaves something open:

  - a row with a non-finite coordinate is dropped and renumbers nothing (the reference casts it to an integer: undefined);
  - the voxels come out in ascending (z, y, x) of their integer triple (the reference: std::unordered_map's order);
  - V3's centroid is the float64 mean of all fields rounded to float32 (pcl::CentroidPoint sums in float, in the map's order);
  - V2's mean is a float32 sum from zero over its kept rows in ascending row index, divided by float32(count);
  - a cloud whose packed key would need more than 64 bits, or in which floor(p * inv) / p / gs leaves the int range, is refused.

Every step the reference takes in float is taken in float32.  A voxel is held in a dict under its integer triple with the list of its rows,
as both classes hold it; the packed key exists beside it for the sort tests.  Nothing here uses oracle/ or the device.

V3:  inv = 1.0f / gs;  min_b = (int)floor(min_p * inv);  ijk = floor(p * inv) - (float)min_b   -- pcl::VoxelGrid's lattice, no too-fine test.
V2:  voxel = (int)(p / gs): a float division truncated toward zero; the first max_voxel_pts rows of a voxel are kept (pcp.hpp:110-116), the
     voxel is emitted when it kept more than min_voxel_pts (:125); the record is the first row's with x, y, z replaced by the mean (:139-147).
Key: per axis the triple relative to its smallest value over the kept rows; an axis of extent e takes bits(e - 1) bits; x lowest, then y, then z.
"""
import numpy as np

V3, V2 = 3, 2
INT_LO, INT_HI = -2.0 ** 31, 2.0 ** 31


class SparseRefused(Exception):
    """what the device must refuse: .why is 'bits' (with .extents and .bits) or 'range'"""

    def __init__(self, why, extents=None, bits=None):
        super().__init__(f"{why} {extents} {bits}")
        self.why, self.extents, self.bits = why, extents, bits


def intensity_column(stride):
    """the channel V3 averages besides x, y, z: float 4 of the 32-byte pcl::PointXYZI, float 3 of a 16- to 28-byte record, none for 12 bytes"""
    return 4 if stride >= 8 else (3 if stride >= 4 else None)


def axis_bits(extent):
    return int(extent - 1).bit_length()


def lattice(pts, leaf, kind):
    """-> (kept mask, (m, 3) float32 lattice values of the kept rows): floor(p * inv) for V3, trunc(p / gs) for V2; refuses what leaves int"""
    p = np.ascontiguousarray(pts, np.float32)
    kept = np.isfinite(p[:, :3]).all(1)
    gs = np.float32(leaf)
    xyz = p[kept, :3]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        f = np.floor(xyz * (np.float32(1.0) / gs)) if kind == V3 else np.trunc(xyz / gs)
    if f.size and not ((f >= INT_LO) & (f < INT_HI)).all():
        raise SparseRefused("range")
    return kept, f.astype(np.float32)


def pack(f, kind):
    """the kept rows' lattice values (m >= 1 rows) -> (relative triples int64, extents, bits per axis, packed keys uint64); refuses > 64 bits"""
    lo = f.min(0)
    if kind == V3:
        rel = (f - lo).astype(np.int64)                          # float32 subtraction: floor(p * inv) - (float)min_b
    else:
        rel = f.astype(np.int64) - lo.astype(np.int64)           # exact integers
    extents = tuple(int(v) + 1 for v in rel.max(0))
    bits = tuple(axis_bits(e) for e in extents)
    if sum(bits) > 64:
        raise SparseRefused("bits", extents, sum(bits))
    sx, sy = bits[0], bits[0] + bits[1]
    keys = np.array([int(x) | (int(y) << sx) | (int(z) << sy) for x, y, z in rel], np.uint64)
    return rel, extents, bits, keys


def sorted_pairs(pts, leaf, kind):
    """-> (keys, rows) of the kept rows as a stable sort by packed key leaves them: what pcr_voxel_sparse_order must hand out"""
    kept, f = lattice(pts, leaf, kind)
    rows = np.flatnonzero(kept)
    if not len(rows):
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    keys = pack(f, kind)[3]
    o = np.argsort(keys, kind="stable")
    return keys[o], rows[o].astype(np.uint32)


class SparseRef:
    """sparse_ref(pts, leaf, kind, max_voxel_pts, min_voxel_pts) -> SparseRef

    kept       bool per input row
    rows       the kept rows' input indices, ascending
    rel        (m, 3) int64: the kept rows' triples relative to the per-axis minimum
    extents    (ex, ey, ez); bits = (bx, by, bz)
    keys       (m,) uint64: the kept rows' packed keys, in input order
    voxels     dict: relative triple (x, y, z) -> list of its input rows, ascending
    out        the filter's output rows, float32, ascending (z, y, x)
    out_rows   V2: per output record the input row whose bytes it carries; V3: the first row of the voxel
    members    per output record the input rows that went into it, ascending
    """

    def __init__(self, pts, leaf, kind=V3, max_voxel_pts=20, min_voxel_pts=0):
        pts = np.ascontiguousarray(pts, np.float32)
        self.pts, self.kind = pts, kind
        n, stride = pts.shape
        self.kept, f = lattice(pts, leaf, kind)
        self.rows = np.flatnonzero(self.kept)
        self.voxels = {}
        self.out = np.zeros((0, stride), np.float32)
        self.out_rows = np.zeros(0, np.int64)
        self.members = []
        self.rel = np.zeros((0, 3), np.int64)
        self.keys = np.zeros(0, np.uint64)
        self.extents, self.bits = (0, 0, 0), (0, 0, 0)
        if not len(self.rows):
            return
        self.rel, self.extents, self.bits, self.keys = pack(f, kind)
        for r, t in zip(self.rows, map(tuple, self.rel)):        # the reference's map: voxel -> its rows, in input order
            self.voxels.setdefault(t, []).append(int(r))
        order = sorted(self.voxels, key=lambda t: (t[2], t[1], t[0]))
        if kind == V3:
            self._centroids(order)
        else:
            self._first_rows_mean(order, int(max_voxel_pts), int(min_voxel_pts))

    def _centroids(self, order):
        stride = self.pts.shape[1]
        ic = intensity_column(stride)
        out = np.zeros((len(order), stride), np.float32)
        first = np.zeros(len(order), np.int64)
        p64 = self.pts.astype(np.float64)
        for i, t in enumerate(order):
            m = self.voxels[t]
            first[i] = m[0]
            out[i, :3] = p64[m, :3].mean(0)
            if ic is not None:
                out[i, ic] = p64[m, ic].mean()
        if stride >= 8:
            out[:, 3] = 1.0                                      # pcl::PointXYZI keeps data[3] = 1
        self.out, self.out_rows, self.members = out, first, [self.voxels[t] for t in order]

    def _first_rows_mean(self, order, max_pts, min_pts):
        recs, rows = [], []
        for t in order:
            m = self.voxels[t][:max_pts]                         # pcp.hpp:115: only while size() < _max_voxel_pts
            if not len(m) > min_pts:                             # pcp.hpp:125: strictly greater
                continue
            s = np.zeros(3, np.float32)
            for r in m:                                          # p.setZero(); p += each, in index order
                s = s + self.pts[r, :3]
            rec = self.pts[m[0]].copy()
            rec[:3] = s / np.float32(len(m))
            recs.append(rec)
            rows.append(m[0])
            self.members.append(m)
        if recs:
            self.out, self.out_rows = np.array(recs, np.float32), np.array(rows, np.int64)

    def sorted_pairs(self):
        """-> (keys, rows) as a stable sort of the kept rows by key leaves them"""
        o = np.argsort(self.keys, kind="stable")
        return self.keys[o], self.rows[o].astype(np.uint32)


def sparse_ref(pts, leaf, kind=V3, max_voxel_pts=20, min_voxel_pts=0):
    return SparseRef(pts, leaf, kind, max_voxel_pts, min_voxel_pts)


def ulp_distance(a, b):
    """|a - b| in float32 ulps, element-wise (both finite float32)"""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def assert_v3(got, ref, what=""):
    """the standing criterion of the voxel-filter tests: the same rows, every averaged channel within one float32 ulp of the float64 mean,
    the constant channels exact"""
    got = np.asarray(got, np.float32)
    assert got.shape == ref.out.shape, f"{what}: {got.shape} vs {ref.out.shape} in the restatement"
    d = ulp_distance(got, ref.out)
    if d.size and d.max() > 1:
        r, c = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError(f"{what}: row {r} col {c}: {got[r, c]!r} vs {ref.out[r, c]!r} ({d[r, c]} ulps); {int((d > 1).any(1).sum())} rows off")


def assert_v2(got, ref, what=""):
    """bit for bit"""
    got = np.asarray(got, np.float32)
    assert got.shape == ref.out.shape, f"{what}: {got.shape} vs {ref.out.shape} in the restatement"
    np.testing.assert_array_equal(got.view(np.uint32), ref.out.view(np.uint32), err_msg=what)
