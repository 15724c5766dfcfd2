"""tests/ndt_voxel_ref.py, the exact reference the device's NDT voxel Gaussians are held to (tests/test_ndt_voxels_gpu.py), against the
oracle's restatement of VoxelGridCovariance (oracle/ndt_oracle.c: oracle_ndt_leaves) on every cloud of tests/ndt_clouds.py -- and the
clouds themselves: each holds the class of voxel it is named for.  No GPU.

(The compiled reference library under oracle/_ref holds the reference's nanoflann only: tests/test_oracle_vgicp_ndt.py reaches no
voxel code through it, so there is nothing of the reference's own to compare the voxels with here.)"""
import numpy as np
import pytest

import ndt_clouds as nc
import ndt_voxel_ref as vr
import oracle

CASES = nc.all_voxel_cases()
_cache = {}


def _both(case):
    name, cloud, res, mp = case
    if name not in _cache:
        ref = vr.exact_voxels(cloud, res, mp)
        o = vr.sort_xyz(oracle.ndt_leaves(cloud, oracle.ndt_params(resolution=res, min_points=mp)))
        _cache[name] = (ref, o)
    return _cache[name]


def _icov_ratio(ref, o):
    kept = o["n"] > 0
    if not kept.any():
        return 0.0
    d = np.abs(o["icov"] - ref["icov"]).reshape(-1, 9).max(axis=1)
    return float((d / vr.icov_bound_unit(ref))[kept].max())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_matches_oracle(case):
    ref, o = _both(case)
    # the same voxels: the lattice, and the min_points threshold with its clamp to 3
    np.testing.assert_array_equal(o["ijk"], ref["ijk"])
    kept = o["n"] > 0
    np.testing.assert_array_equal(o["n"][kept], ref["n"][kept])
    # the verdict (:337-341) is the exact one wherever the exact covariance is not singular: a singular one is kept or dropped on the
    # rounding of whoever evaluates it
    regular = ref["lam_min"] > 1e-9 * ref["lam_max"]
    np.testing.assert_array_equal(kept[regular], ref["kept"][regular])
    if not case[0].startswith(("shaky", "threshold-min3", "threshold-min1")):
        assert regular.all()
    assert (np.abs(o["mean"] - ref["mean"]).max(axis=1) <= vr.mean_bound(ref)).all()
    r = _icov_ratio(ref, o)
    print(f"{case[0]}: voxels {len(kept)} kept {int(kept.sum())} largest (oracle - exact) / bound unit = {r:.3f}")
    assert r <= vr.ICOV_K_MEASURED * 1.0001


def test_oracle_error_sets_K():
    """K of the icov bound is not chosen: it is four times the oracle's own largest error in units of
    2^-53 n R^2 / lam_min(clamped) ||icov||_max.  Measured here: 0.225 (generic-origin-0.5); per cloud 0.16 generic-origin-1.0,
    0.12 -1.5, 0.08 -2.0, shifted 0.09 / 0.19 / 0.12 / 0.13, threshold 0.17, crowded 0.07, binary 0.14, shaky 0.22, faces 0.17.
    (The figure is printed; only its staying below the recorded value is asserted: numpy's eigh may move it a little.)"""
    worst = max(_icov_ratio(*_both(c)) for c in CASES)
    print(f"largest oracle error over all clouds: {worst:.4f} bound units; K = {vr.ICOV_K}")
    assert worst <= vr.ICOV_K_MEASURED * 1.0001
    assert vr.ICOV_K == 4 * vr.ICOV_K_MEASURED


def _case(name):
    return next(c for c in CASES if c[0] == name)


def test_generic_holds_every_clamp_outcome_and_the_edge_of_the_clamp():
    for tag in ("origin", "shifted"):
        ref, _ = _both(_case(f"generic-{tag}-1.0"))
        assert len(ref["n"]) == 294 and ref["n"].min() >= 6 and ref["n"].max() <= 40
        counts = np.bincount(ref["raised"], minlength=3)
        assert (counts >= 50).all(), counts                      # unclamped, clamped once, clamped twice
        w = np.linalg.eigvalsh(ref["cov"])
        ratio = w[:, :2] / w[:, 2:]
        assert ((ratio > 0.008) & (ratio < 0.01)).sum() >= 3 and ((ratio > 0.01) & (ratio < 0.0125)).sum() >= 3      # just either side of 0.01
    ref, _ = _both(_case("generic-shifted-1.0"))
    assert ref["R"].min() > 395.0                                 # where the about-the-origin formula cancels hardest


def test_threshold_holds_3_5_6_7_and_the_clamp_of_min_points():
    for mp, want in ((6, {6: 10, 7: 10}), (3, {3: 10, 5: 10, 6: 10, 7: 10}), (1, {3: 10, 5: 10, 6: 10, 7: 10})):
        ref, o = _both(_case(f"threshold-min{mp}"))
        got = {int(n): int(c) for n, c in zip(*np.unique(ref["n"], return_counts=True))}
        assert got == want, (mp, got)
    assert int((_both(_case("threshold-min3"))[1]["n"] < 0).sum()) >= 1      # three points span a plane: some are rejected


def test_crowded_runs_both_sum_paths_on_both_sides_of_the_bound():
    for res, (below, above) in ((1.0, (512, 513)), (2.0, (256, 257))):
        ref, _ = _both(_case(f"crowded-{res}"))
        assert sorted(ref["n"].tolist()) == sorted(nc.CROWDED_COUNTS)
        i64 = nc.on_int64_path(ref["n"].astype(float), res)
        assert not i64[ref["n"] == below][0] and i64[ref["n"] == above][0]
        assert i64.sum() >= 3 and (~i64).sum() >= 1, (res, i64)
        assert i64[ref["n"] == 4097][0] and i64[ref["n"] == 700][0]


def test_binary_is_on_its_lattice_with_unclamped_voxels():
    cloud = _case("binary")[1]
    assert (cloud[:, :3] / nc.LATTICE == np.round(cloud[:, :3] / nc.LATTICE)).all() and np.abs(cloud[:, :3]).max() <= 64.0
    ref, o = _both(_case("binary"))
    assert len(ref["n"]) == 200 and (ref["raised"] == 0).sum() >= 40 and (ref["raised"] > 0).sum() >= 40
    # its sums are exact in double: the oracle's mean IS the exact one
    np.testing.assert_array_equal(o["mean"], ref["mean"])


def test_shaky_is_singular_and_its_verdicts_depend_on_the_order():
    cloud, perms = nc.shaky()
    refs = [_both(_case(f"shaky-perm{k}")) for k in range(3)]
    ref = refs[0][0]
    assert (ref["lam_min"] <= 1e-9 * ref["lam_max"]).all()       # every voxel
    got = {int(n): int(c) for n, c in zip(*np.unique(ref["n"], return_counts=True))}
    assert set(got) == set(nc.SHAKY_COUNTS) and all(got[n] >= 8 for n in nc.SHAKY_COUNTS), got
    on_lattice = np.array([(cloud[(np.floor(cloud[:, :3]) == ijk).all(1), :3] / nc.LATTICE % 1 == 0).all() for ijk in ref["ijk"]])
    assert on_lattice[ref["n"] > 64].all() and (~on_lattice).sum() == 36
    kept = np.array([r[1]["n"] > 0 for r in refs])
    assert kept.any() and (~kept).any()
    assert (kept[:, on_lattice] == kept[0, on_lattice]).all()    # exact sums: no order
    assert (kept[:, ~on_lattice] != kept[0, ~on_lattice]).any()  # off the lattice the order decides


@pytest.mark.parametrize("leaf", nc.FACES_LEAVES)
def test_faces_has_members_the_two_roundings_place_differently(leaf):
    cloud, probes = nc.faces(leaf)
    built = vr.lattice(probes, leaf)[1][:, 0]
    looked = vr.lattice_lookup(probes, leaf)[:, 0]
    k = np.repeat(list(range(-24, 0)) + list(range(1, 25)), 3)
    assert ((built == k) | (built == k - 1)).all() and ((looked == k) | (looked == k - 1)).all()
    assert (built != looked).sum() >= 3, (leaf, int((built != looked).sum()))
    assert (built[k < 0] != looked[k < 0]).any() or (built[k > 0] != looked[k > 0]).any()
    # company: both voxels of every face qualify
    ref, o = _both(_case(f"faces-{leaf}"))
    have = {tuple(v) for v in ref["ijk"][o["n"] >= 6]}
    rows = np.floor(probes[:, 1].astype(np.float32) * (np.float32(1) / np.float32(leaf))).astype(int)
    for kk, row in zip(k[::3], rows[::3]):
        assert (kk - 1, row, 0) in have and (kk, row, 0) in have, (kk, row)


def test_unclean_rows_belong_to_no_voxel():
    u = nc.unclean()
    assert (~np.isfinite(u["mixed"][:, :3])).any(axis=1).sum() == 40
    ref, o = _both(_case("unclean-mixed"))
    clean, oc = _both(_case("threshold-min6"))
    for k in ("ijk", "n", "mean", "icov"):
        np.testing.assert_array_equal(o[k], oc[k])
    assert len(_both(_case("unclean-five"))[0]["n"]) == 0 and len(_both(_case("unclean-empty"))[0]["n"]) == 0
