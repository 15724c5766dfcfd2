"""Small seeded NDT targets, one per class of voxel that ndt_voxel_kernel (csrc/ndt.hip) treats differently.  A few thousand points and a
few hundred voxels each; tests/test_ndt_voxel_ref.py counts that every class is really there, tests/test_ndt_voxels_gpu.py and
tests/test_ndt_sums_gpu.py run the device on them.  Every cloud is (n, 4) float32, w = 0."""
import numpy as np

LATTICE = 2.0 ** -10       # the binary lattice of `binary` and `shaky`


def _xyz0(p):
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = np.asarray(p, np.float64)
    return out


def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def _blob(rng, n, centre, sig, half=0.45):
    """n points of an oriented Gaussian about centre, kept inside centre +- half"""
    x = (rng.standard_normal((n, 3)) * sig) @ _rot(rng).T
    return centre + np.clip(x, -half, half)


# standard deviations along the three axes of a blob.  The clamp raises an eigenvalue below 0.01 of the largest, i.e. an axis whose
# deviation is below a tenth of the longest one: the "edge" shapes sit at 0.1 * (1 +- 0.1), where a handful of samples falls either side.
_SHAPES = [
    (0.20, 0.15, 0.10), (0.20, 0.10, 0.05),                       # no eigenvalue raised
    (0.20, 0.10, 0.005), (0.20, 0.06, 0.002),                     # one raised
    (0.20, 0.005, 0.003), (0.20, 0.002, 0.002),                   # two raised
    (0.20, 0.10, 0.022), (0.20, 0.10, 0.018), (0.20, 0.022, 0.018), (0.20, 0.019, 0.021),      # either side of the ratio 0.01
]


def generic(shift=(0.0, 0.0, 0.0)):
    """294 voxels of 1 m (7 x 7 x 6), 6..40 points each, blobs of mixed anisotropy; optionally moved far from the origin"""
    rng = np.random.default_rng(1201)
    parts = []
    k = 0
    for iz in range(6):
        for iy in range(7):
            for ix in range(7):
                n = int(rng.integers(6, 41))
                parts.append(_blob(rng, n, np.array([ix + 0.5, iy + 0.5, iz + 0.5]) - 3.0, np.array(_SHAPES[k % len(_SHAPES)])))
                k += 1
    p = np.concatenate(parts) + np.asarray(shift, np.float64)
    return _xyz0(p[rng.permutation(len(p))])


GENERIC_SHIFT = (400.0, -300.0, 20.0)
GENERIC_RESOLUTIONS = (1.0, 0.5, 1.5, 2.0)


def threshold():
    """ten voxels each with exactly 3, 5, 6 and 7 points (1 m voxels, every other cell along x)"""
    rng = np.random.default_rng(1202)
    parts = []
    for row, n in enumerate((3, 5, 6, 7)):
        for k in range(10):
            parts.append(np.array([2 * k + 0.5, 2 * row + 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (n, 3)))
    p = np.concatenate(parts)
    return _xyz0(p[rng.permutation(len(p))])


THRESHOLD_MIN_POINTS = (6, 3, 1)
CROWDED_COUNTS = (512, 513, 700, 300, 4097, 256, 257)


def crowded():
    """One voxel per count of CROWDED_COUNTS, each inside one 1 m cell whose 2 m cell holds nothing else.  The kernel adds the fixed-point
    terms up as doubles while n * cell <= 512 and n * cell^2 <= 16384 and as int64 beyond: at 1 m 512 | 513 straddle the first bound, at
    2 m 256 | 257 do (300 and 4097 lie beyond it; n * cell^2 binds only for cells above 32 m, where n * cell has been passed long before)."""
    rng = np.random.default_rng(1203)
    parts = []
    for k, n in enumerate(CROWDED_COUNTS):
        parts.append(np.array([4 * k + 0.5, 0.5, 0.5]) + (rng.uniform(-0.45, 0.45, (n, 3)) * np.array([1.0, 0.5, 0.2])) @ _rot(rng).T * 0.7)
    p = np.concatenate(parts)
    return _xyz0(p[rng.permutation(len(p))])


CROWDED_RESOLUTIONS = (1.0, 2.0)


def on_int64_path(n, cell):
    return (n * cell > 512.0) | (n * cell * cell > 16384.0)


def binary():
    """200 voxels of 1 m inside +-64 m whose coordinates are multiples of 2^-10: sums of x and x x^T are exact in double in any order"""
    rng = np.random.default_rng(1204)
    cells = set()
    while len(cells) < 200:
        cells.add((int(rng.integers(-64, 64)), int(rng.integers(-8, 8)), int(rng.integers(-2, 2))))
    parts = []
    for k, c in enumerate(sorted(cells)):
        n = int(rng.integers(6, 31))
        x = _blob(rng, n, np.array(c) + 0.5, np.array(_SHAPES[k % len(_SHAPES)]), half=0.45)
        parts.append(np.round(x / LATTICE) * LATTICE)
    p = np.concatenate(parts)
    return _xyz0(p[rng.permutation(len(p))])


SHAKY_COUNTS = (6, 12, 64, 65, 80)
SHAKY_RESUMMED = (6, 12, 64)       # n <= 64: a voxel that is singular but for rounding is summed again in input order


def shaky():
    """Voxels whose covariance is singular in exact arithmetic, so that keeping them hangs on rounding: three distinct points repeated,
    collinear points, an axis-aligned and a tilted flat patch -- on the binary lattice for every n of SHAKY_COUNTS, and (n <= 64 only, where
    the kernel follows the reference's summation order) once more with coordinates off the lattice, where that order decides.
    Returns (cloud, three permutations of its rows)."""
    rng = np.random.default_rng(1205)
    parts = []
    cell = 0

    def centre():
        nonlocal cell
        c = np.array([2 * (cell % 12) + 0.5, 2 * (cell // 12) + 0.5, 0.5])
        cell += 1
        return c

    def snap(x):
        return np.round(x / LATTICE) * LATTICE

    for n in SHAKY_COUNTS:
        for rep in range(2):
            three = snap(centre() + rng.uniform(-0.4, 0.4, (3, 3)))
            parts.append(three[np.arange(n) % 3])                                                   # three points, repeated
            c = centre()
            d = np.array([3, 2, 1]) * LATTICE * (1 + rep)
            parts.append(snap(c) + (np.arange(n) - n // 2)[:, None] * d)                            # collinear
            f = snap(centre() + rng.uniform(-0.4, 0.4, (n, 3))); f[:, 2] = f[0, 2]
            parts.append(f)                                                                         # flat, normal along z
            c = snap(centre())
            u = np.round(rng.uniform(-0.3, 0.3, (n, 2)) / (2 * LATTICE)) * (2 * LATTICE)
            parts.append(c + np.stack([u[:, 0], u[:, 1], 0.5 * u[:, 0]], 1))                        # flat, tilted: z = x / 2
    for n in SHAKY_RESUMMED:
        for rep in range(12):
            three = centre() + rng.uniform(-0.3, 0.3, (3, 3)) + 0.1234567
            parts.append(three[rng.permutation(np.arange(n) % 3)])                                  # off the lattice
    p = _xyz0(np.concatenate(parts))
    perms = [np.arange(len(p)), rng.permutation(len(p)), rng.permutation(len(p))]
    return p, perms


FACES_LEAVES = (1.5, 0.3)


def faces(leaf):
    """Along x: for every face k * leaf, k = +-1 .. +-24, the point exactly on it and one float32 ulp either side (y, z in the middle of
    a cell of its own row), with eight points of company in each of the two voxels the face separates.  Returns (cloud, the face points)."""
    rng = np.random.default_rng(1206)
    lf = np.float32(leaf)
    parts, px, py = [], [], []
    for row, k in enumerate(list(range(-24, 0)) + list(range(1, 25))):
        f = np.float32(k) * lf
        y = (row + 0.5) * leaf
        px += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        py += [y, y, y]
        for side in (-0.5, 0.5):
            parts.append(np.array([(k + side) * leaf, y, 0.5 * leaf]) + rng.uniform(-0.3, 0.3, (8, 3)) * leaf)
    probes = np.zeros((len(px), 4), np.float32)
    probes[:, 0] = np.array(px, np.float32)      # (float32 all the way: the ulp must survive)
    probes[:, 1] = np.array(py)
    probes[:, 2] = 0.5 * leaf
    cloud = np.concatenate([_xyz0(np.concatenate(parts)), probes])
    return cloud[rng.permutation(len(cloud))], probes


def unclean():
    """the `threshold` cloud with NaN / inf rows mixed in (they belong to no voxel), a target of five points, an empty target"""
    rng = np.random.default_rng(1207)
    base = threshold()
    bad = np.zeros((40, 4), np.float32)
    bad[:, :3] = rng.uniform(0, 8, (40, 3))
    bad[np.arange(40), rng.integers(0, 3, 40)] = np.tile(np.array([np.nan, np.inf, -np.inf, np.nan], np.float32), 10)
    mixed = np.concatenate([base, bad])
    mixed = mixed[rng.permutation(len(mixed))]
    five = _xyz0(np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (5, 3)))
    return dict(mixed=mixed, five=five, empty=np.zeros((0, 4), np.float32))


def room(n=3000):
    """floor and two walls of a 10 x 10 x 3 m room, dense enough for 1 m voxels (as tests/test_loam_refine_gpu.py's room)"""
    rng = np.random.default_rng(1208)
    k = n // 3
    floor = np.stack([rng.uniform(0, 10, k), rng.uniform(0, 10, k), rng.normal(0, 0.01, k)], 1)
    wall_x = np.stack([rng.normal(0, 0.01, k), rng.uniform(0, 10, k), rng.uniform(0, 3, k)], 1)
    wall_y = np.stack([rng.uniform(0, 10, n - 2 * k), rng.normal(0, 0.01, n - 2 * k), rng.uniform(0, 3, n - 2 * k)], 1)
    return _xyz0(np.concatenate([floor, wall_x, wall_y]))


ROOM_SCAN_SIZES = (129, 513, 1025)


def room_scan_case(n):
    """(target, scan, guess) of a small alignment: the room, n of its points with 1 cm of noise, a guess 5 cm and 0.3 degrees off the identity"""
    from simpleslam_amd import synth
    m = room()
    rng = np.random.default_rng([1209, n])
    scan = m[rng.choice(len(m), n, replace=False)].copy()
    scan[:, :3] += rng.normal(0.0, 0.01, (n, 3)).astype(np.float32)
    return m, scan, synth.perturb(np.eye(4), 1209 + n, trans=0.05, rot_deg=0.3)


def all_voxel_cases():
    """(name, cloud, resolution, min_points) of every voxel comparison"""
    cases = []
    for tag, sh in (("origin", (0, 0, 0)), ("shifted", GENERIC_SHIFT)):
        g = generic(sh)
        for res in GENERIC_RESOLUTIONS:
            cases.append((f"generic-{tag}-{res}", g, res, 6))
    t = threshold()
    for mp in THRESHOLD_MIN_POINTS:
        cases.append((f"threshold-min{mp}", t, 1.0, mp))
    c = crowded()
    for res in CROWDED_RESOLUTIONS:
        cases.append((f"crowded-{res}", c, res, 6))
    cases.append(("binary", binary(), 1.0, 6))
    s, perms = shaky()
    for k, pm in enumerate(perms):
        cases.append((f"shaky-perm{k}", s[pm], 1.0, 6))
    for leaf in FACES_LEAVES:
        cases.append((f"faces-{leaf}", faces(leaf)[0], leaf, 6))
    u = unclean()
    for k in ("mixed", "five", "empty"):
        cases.append((f"unclean-{k}", u[k], 1.0, 6))
    return cases
