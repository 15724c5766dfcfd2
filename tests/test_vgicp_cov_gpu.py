"""VGICP's per-point covariances on every kernel path, and the voxel fold on both of its branches, against the plain reference of
tests/cov_ref.py (brute-force neighbours, long double scatter, LAPACK's eigenvectors).

- scan-sized clouds (n <= 300 000): csrc/cov_search.hip (cov_ring1_kernel, cov_wave_kernel, cov_from_nbr_kernel);
- map-sized clouds: csrc/vgicp.hip: vgicp_cov_kernel<false>, lane per query, one search level;
- csrc/vgicp.hip: vgicp_voxel_kernel, doubles while cnt * max(cell, 1) <= 256 and long long beyond.

The measure is err * gap and the bound cov_ref.DEVICE_ERR_GAP_BOUND: ten times what the CPU oracle itself shows against the reference
(tests/test_cov_ref.py), never a figure taken from the kernels.  Each test prints what it observed."""
import numpy as np
import pytest

import cov_ref
from simpleslam_amd import VgicpRegister

pytestmark = pytest.mark.gpu

NAMES = ["lattice", "plane", "tilted", "line", "far_plane", "blob", "lidar", "two_planes", "clump"]
DEGENERATE = ["lattice", "plane", "tilted", "line", "far_plane", "two_planes", "clump"]


def _check(got, ref, label):
    """every query that is not `ambiguous` within the bound on err * gap; every matrix symmetric with eigenvalues (1e-3, 1, 1) to 1e-12"""
    keep = ~ref.ambiguous
    eg = cov_ref.err_gap(got, ref)
    ev, asym = cov_ref.eigenvalue_error(got)
    print(f"{label}: max err*gap {eg[keep].max():.3e} (bound {cov_ref.DEVICE_ERR_GAP_BOUND:.1e}), raw error {np.abs(got - ref.cov)[keep].max():.3e}, "
          f"smallest gap {ref.gap.min():.2e}, ambiguous {int(ref.ambiguous.sum())} of {len(keep)}, gap <= floor {int((ref.gap <= cov_ref.GAP_FLOOR).sum())}, "
          f"eigenvalues off by {ev:.2e}")
    assert np.isfinite(got).all(), label
    over = keep & ~(eg <= cov_ref.DEVICE_ERR_GAP_BOUND)
    assert not over.any(), (label, int(over.sum()), float(eg[keep].max()), np.flatnonzero(over)[:8])
    assert ev <= 1e-12 and asym == 0.0, (label, ev, asym)
    return float(eg[keep].max())


# ---------------------------------------------------------------------------
# scan-sized path
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_path(gpu):
    """name -> (covariances, neighbour lists, queries that went to the wave kernel), one fresh handle each"""
    out = {}
    for name in NAMES:
        reg = VgicpRegister()
        pts = cov_ref.clouds()[name]
        cov = reg.covariances(pts)
        out[name] = (cov,) + reg.neighbours(len(pts))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_scan_sized_path_matches_the_reference(scan_path, name):
    cov, nb, queued = scan_path[name]
    ref = cov_ref.reference(name)
    clear = ~ref.ambiguous
    assert (nb[clear] == ref.idx[clear]).all(), int((nb != ref.idx).any(axis=1).sum())      # the lists themselves, (distance, index) order
    _check(cov, ref, f"scan-sized {name} (wave kernel: {queued} of {len(cov)})")


def test_both_classes_of_queries_occurred(scan_path):
    queued = {name: (scan_path[name][2], len(scan_path[name][0])) for name in NAMES}
    print(queued)
    assert any(0 < q < n for q, n in queued.values()), queued


@pytest.mark.parametrize("name", ["lattice", "lidar"])
def test_device_tensors_and_32_byte_rows_give_the_same_bits(scan_path, name):
    import torch
    pts = cov_ref.clouds()[name]
    wide = np.zeros((len(pts), 8), np.float32)             # pcl::PointXYZI: x y z pad intensity pad pad pad
    wide[:, :3] = pts[:, :3]
    wide[:, 4] = 0.5
    host16 = scan_path[name][0]
    for label, cloud in (("device 16", torch.from_numpy(np.array(pts)).cuda()), ("host 32", wide), ("device 32", torch.from_numpy(wide).cuda())):
        got = VgicpRegister().covariances(cloud)
        assert np.array_equal(got, host16), (name, label, int((got != host16).any(axis=(1, 2)).sum()))


# ---------------------------------------------------------------------------
# map-sized path
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def map_case(gpu):
    """The cluster map, the reference of >= 4 000 of its queries (each brute-forced inside its own cluster, which the separation asserted here
    makes the whole cloud's answer) and the device's covariances: a handle's first call, and another handle's first and second."""
    m, clusters = cov_ref.cluster_map()
    assert 300_000 < len(m) <= 303_000
    rng = np.random.default_rng(61)
    seen, refs = set(), []
    for q, (kind, a, b) in enumerate(clusters):
        if kind in DEGENERATE and kind not in seen:
            seen.add(kind)
            rows = np.arange(b - a)
        else:
            rows = np.sort(rng.choice(b - a, 10, replace=False))
        r = cov_ref.covariances(m[a:b], rows)
        # in-cluster brute force is the whole cloud's: the 21st in-cluster neighbour is nearer than any point of another cluster can be
        assert (np.sqrt(r.d2[:, 20].astype(np.float64)) < cov_ref.distance_to_other_clusters(m[a:b][rows], q)).all(), (q, kind)
        refs.append((q, kind, a + rows, r))
    assert seen == set(DEGENERATE) and sum(len(rows) for _, _, rows, _ in refs) >= 4000
    first = VgicpRegister().covariances(m)
    reg = VgicpRegister()
    other = reg.covariances(m)
    again = reg.covariances(m)
    return dict(map=m, clusters=clusters, refs=refs, first=first, other=other, again=again)


def test_map_sized_path_matches_the_reference(map_case):
    worst = {}
    for q, kind, rows, r in map_case["refs"]:
        got = map_case["first"][rows]
        if len(rows) > 10:
            worst[kind] = _check(got, r, f"map-sized {kind} (cluster {q})")
        else:
            keep = ~r.ambiguous
            eg = cov_ref.err_gap(got, r)
            assert (eg[keep] <= cov_ref.DEVICE_ERR_GAP_BOUND).all(), (q, kind, float(eg.max()))
            worst["sample"] = max(worst.get("sample", 0.0), float(eg[keep].max()) if keep.any() else 0.0)
    print("map-sized path, max err*gap:", {k: f"{v:.3e}" for k, v in worst.items()})
    ev, asym = cov_ref.eigenvalue_error(map_case["first"])      # every point of the map
    assert ev <= 1e-12 and asym == 0.0, (ev, asym)


def test_map_sized_path_is_the_same_on_every_call(map_case):
    """a handle's second call (hints of the first at work) and another handle's first: bit for bit"""
    assert np.array_equal(map_case["other"], map_case["first"])
    assert np.array_equal(map_case["again"], map_case["first"])


def test_the_two_paths_give_the_same_bits(map_case):
    """One cluster inside the map-sized cloud and alone (scan-sized): the arithmetic after the search is one function (cov_math.h), so every
    point whose 21 nearest lie in the cluster either way gets the same matrix bit for bit."""
    m = map_case["map"]
    checked = 0
    for q, (kind, a, b) in enumerate(map_case["clusters"][:9]):
        alone = VgicpRegister().covariances(np.ascontiguousarray(m[a:b]))
        _, d2 = cov_ref.neighbours(m[a:b])
        inside = np.sqrt(d2[:, 20].astype(np.float64)) < cov_ref.distance_to_other_clusters(m[a:b], q)
        assert inside.mean() > 0.99, (kind, inside.mean())
        differ = (alone != map_case["first"][a:b]).any(axis=(1, 2)) & inside
        assert not differ.any(), (kind, int(differ.sum()), np.flatnonzero(differ)[:8])
        checked += int(inside.sum())
    assert checked > 15_000


# ---------------------------------------------------------------------------
# voxel fold, both branches
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold_case():
    m = cov_ref.fold_map()
    s = cov_ref.fold_scan(m)
    return dict(map=m, scan=s, map_cov=cov_ref.covariances(m), scan_cov=cov_ref.covariances(s))


@pytest.mark.parametrize("res", [1.0, 0.5, 2.0])
def test_voxel_fold_matches_the_transcription(gpu, fold_case, res):
    """VgicpRegister.linearize against cov_ref.linearize fed with cov_ref's covariances.  Resolution 1.0: voxels of 1, 2, about 25 points
    (doubles) and of 400, 900 and 1 000 (long long); 0.5: 700 in one voxel; 2.0: 200 points in one voxel, 200 * 2.0 > 256 through the
    cell > 1 side.  H, b and the error within cov_ref.DEVICE_LIN_BOUND -- ten times the CPU oracle's own distance from the same transcription --
    and bit for bit the same when the map's rows are permuted: the fixed-point sums do not depend on the order."""
    m, s, rm, rs = fold_case["map"], fold_case["scan"], fold_case["map_cov"], fold_case["scan_cov"]
    cnt = cov_ref.voxel_counts(m, res)
    if res == 1.0:
        assert (cnt == 1).sum() >= 20 and (cnt == 2).sum() >= 10 and ((cnt >= 15) & (cnt <= 40)).sum() >= 4
        assert ((cnt >= 300) & (cnt <= 2000)).sum() >= 3
    elif res == 0.5:
        assert cnt.max() > 600
    else:
        assert (cnt == 200).sum() == 1 and (cnt * res <= 256).any() and (cnt * res > 256).any()
    assert (cnt * max(res, 1.0) > 256).any() and (cnt * max(res, 1.0) <= 256).any()      # both branches of the fold
    assert (np.diff(rm.d2, axis=1) > 0).all()      # no two distances of a list equal: neither a list nor its order depends on the order of the rows
    perm = np.random.default_rng(62).permutation(len(m))
    reg, reg_p = VgicpRegister(vgicp_resolution=res), VgicpRegister(vgicp_resolution=res)
    reg.setTarget(m)
    reg_p.setTarget(np.ascontiguousarray(m[perm]))
    on_face = np.floor(s[-20:, :3].astype(np.float64) / res - 0.5) == s[-20:, :3].astype(np.float64) / res - 0.5
    assert on_face.any(axis=1).sum() >= 3
    for T in cov_ref.fold_poses():
        want = cov_ref.linearize(s, m, T, rs.cov, rm.cov, res)
        got = reg.linearize(s, T)
        assert got["n"] == want["n"] >= 300
        d = cov_ref.lin_diff(got, want)
        print(f"voxel fold, resolution {res}: n {got['n']}, H {d[0]:.3e} b {d[1]:.3e} err {d[2]:.3e} (bounds {cov_ref.DEVICE_LIN_BOUND})")
        assert d[0] <= cov_ref.DEVICE_LIN_BOUND[0] and d[1] <= cov_ref.DEVICE_LIN_BOUND[1] and d[2] <= cov_ref.DEVICE_LIN_BOUND[2], d
        got_p = reg_p.linearize(s, T)
        assert got_p["n"] == got["n"] and got_p["err"] == got["err"]
        assert np.array_equal(got_p["H"], got["H"]) and np.array_equal(got_p["b"], got["b"])
