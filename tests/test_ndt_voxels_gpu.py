"""ndt_voxel_kernel (csrc/ndt.hip, "N1") voxel by voxel: the Gaussians read back with pcr_ndt_voxels against the oracle's
(oracle.ndt_leaves: which voxels exist, their n, the keep / drop verdict) and against the exact reference of tests/ndt_voxel_ref.py
(mean, icov), on the clouds of tests/ndt_clouds.py -- one per branch of the kernel: both sum paths, the re-summation in input order, the
clamp with one and two eigenvalues raised, the rejections, min_points and its clamp to 3, the float lattice at faces.  Every voxel of
every cloud is compared.

Bounds (tests/ndt_voxel_ref.py, where each is derived).
  mean   4 * 2^-53 * R, R = the voxel's largest |coordinate|: the formula sum / n with an exact sum rounds three times.  The kernel's
         first moments are exact on every lattice (a float32 leaf makes every voxel centre dyadic), so nothing is added -- on the device
         the mean of every voxel of every cloud here, leaf 0.3 included, equals the exact mean rounded to double: 0 ulps.
  icov   K * 2^-53 * n * R^2 / lam_min(clamped) * ||icov||_max + 9 * 2^-41 / lam_min(clamped) * ||icov||_max per voxel.
         K is not picked: the oracle's own largest error in units of the first term over all the clouds here is 0.225
         (tests/test_ndt_voxel_ref.py::test_oracle_error_sets_K), and the device gets four times that, K = 0.9 -- it feeds its sums into the
         same cancelling expression, but its eigenvectors come from another solver.  The second term is the kernel's fixed-point grid: products
         of centred coordinates are rounded to multiples of 2^-40, and float32 coordinates below 8 m are finer than that.  It is derived from
         the grid alone and added for every voxel; beyond ~20 m from the origin it is small beside the first.  In units of the first term
         alone the device reaches 362 on the generic cloud about the origin at 0.5 m voxels (153 at 1 m; R <= 3.5 m) and 0.19 on the same
         cloud shifted to 400 m, where the products are on the grid: this quantisation is the "1e-10" by which the voxel Gaussians used to
         be said to agree.
  re-summed voxels (n <= 64, singular but for rounding): their sums are the oracle's bit for bit, so their icov is held to the ORACLE's at
         16 * 2^-53 * lam_max / lam_min(clamped) * 3 ||icov||_max, the difference two backward-stable eigen-solvers may leave."""
import numpy as np
import pytest

import ndt_clouds as nc
import ndt_voxel_ref as vr
import oracle
from simpleslam_amd import NdtRegister

pytestmark = pytest.mark.gpu

CASES = nc.all_voxel_cases()
_refs = {}


def _reference(case):
    """the exact reference and the oracle's leaves of a case: computed once, shared, never written to"""
    name, cloud, res, mp = case
    if name not in _refs:
        ref = vr.exact_voxels(cloud, res, mp)
        o = vr.sort_xyz(oracle.ndt_leaves(cloud, oracle.ndt_params(resolution=res, min_points=mp)))
        for d in (ref, o):
            for a in d.values():
                a.setflags(write=False)
        _refs[name] = (ref, o)
    return _refs[name]


def _device(case, reg=None):
    name, cloud, res, mp = case
    reg = reg or NdtRegister(ndt_resolution=res, ndt_min_points=mp)
    reg.setTarget(cloud)
    return reg.voxels()


def _compare(case, dev):
    """every voxel of the case; returns the largest mean and icov errors in units of their bounds"""
    ref, o = _reference(case)
    kept = o["n"] > 0
    # the voxel set, ijk and n: the oracle's, exactly -- the lattice and the keep / drop decision
    np.testing.assert_array_equal(dev["ijk"], o["ijk"][kept])
    np.testing.assert_array_equal(dev["n"], o["n"][kept])
    assert dev["rejected"] == int((~kept).sum())
    if not kept.any():
        return 0.0, 0.0
    sub = {k: v[kept] for k, v in ref.items()}
    me = np.abs(dev["mean"] - sub["mean"]).max(axis=1) / vr.mean_bound(sub)
    mu = np.abs(dev["mean"] - sub["mean"]).max(axis=1) / (vr.EPS * sub["R"])
    err = np.abs(dev["icov"] - sub["icov"]).reshape(-1, 9).max(axis=1)
    ie = err / (vr.ICOV_K * vr.icov_bound_unit(sub) + vr.icov_quantum_bound(sub))
    print(f"{case[0]}: {int(kept.sum())} voxels, mean error {mu.max():.2f} ulps of R = {me.max():.3f} of its bound, icov error {ie.max():.3f} of its bound "
          f"({(err / vr.icov_bound_unit(sub)).max():.3f} units of the first term alone; the oracle's worst is {vr.ICOV_K_MEASURED})")
    assert (me <= 1.0).all(), (case[0], dev["ijk"][me > 1.0][:5], me.max())
    assert (ie <= 1.0).all(), (case[0], dev["ijk"][ie > 1.0][:5], ie.max())
    return float(me.max()), float(ie.max())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_voxel_against_the_oracle_and_the_exact_reference(gpu, case):
    dev = _device(case)
    _compare(case, dev)
    if case[0].startswith("crowded"):      # both sum paths ran, and are held to the same reference
        i64 = nc.on_int64_path(dev["n"].astype(float), case[2])
        assert i64.any() and (~i64).any()


def test_binary_lattice_is_bit_equal_to_the_oracle(gpu):
    """Coordinates on a binary lattice: the sums are exact on both sides and the expressions that follow are the same, so mean and -- where
    no eigenvalue is raised, i.e. no eigenvector enters -- icov are the oracle's bit for bit."""
    case = next(c for c in CASES if c[0] == "binary")
    ref, o = _reference(case)
    dev = _device(case)
    np.testing.assert_array_equal(dev["ijk"], o["ijk"])
    np.testing.assert_array_equal(dev["mean"], o["mean"])
    plain = ref["raised"] == 0
    assert plain.sum() >= 40
    np.testing.assert_array_equal(dev["icov"][plain], o["icov"][plain])


def test_shaky_voxels_in_three_input_orders(gpu):
    """Voxels that are singular but for rounding.  Up to 64 points they are summed again in input order: the device's sums then ARE the
    oracle's on that order -- same voxel set and n (test_every_voxel..., per permutation), the same mean bit for bit, and an icov that
    differs from the oracle's by the two eigen-solvers alone (vr.icov_solver_bound), far inside the bound against the exact reference.
    Beyond 64 points the sums are order independent: the same bits whatever the order."""
    cases = [c for c in CASES if c[0].startswith("shaky-perm")]
    devs = [_device(c) for c in cases]
    big = [d["n"] > 64 for d in devs]
    assert big[0].sum() >= 4      # (16 such voxels in the cloud; the oracle keeps the ones whose rounding came out non-negative)
    for d, b in zip(devs[1:], big[1:]):
        np.testing.assert_array_equal(d["ijk"][b], devs[0]["ijk"][big[0]])
        np.testing.assert_array_equal(d["mean"][b], devs[0]["mean"][big[0]])
        np.testing.assert_array_equal(d["icov"][b], devs[0]["icov"][big[0]])
    for c, d in zip(cases, devs):
        ref, o = _reference(c)
        kept = o["n"] > 0
        small = d["n"] <= 64
        assert small.sum() >= 4
        np.testing.assert_array_equal(d["mean"][small], o["mean"][kept][small])
        sub = {k: v[kept][small] for k, v in ref.items()}
        err = np.abs(d["icov"][small] - o["icov"][kept][small]).reshape(-1, 9).max(axis=1) / vr.icov_solver_bound(sub)
        print(f"{c[0]}: {int(small.sum())} re-summed voxels, icov against the oracle's: {err.max():.3f} of the solver bound")
        assert (err <= 1.0).all(), (c[0], d["ijk"][small][err > 1.0][:5], err.max())


def test_another_target_and_back_returns_the_same_bits(gpu):
    """the two candidate counters used alternately (ndt_candidates_kernel) and the slot table, written in full by every target"""
    a = next(c for c in CASES if c[0] == "generic-origin-1.0")
    b = next(c for c in CASES if c[0] == "crowded-1.0")
    reg = NdtRegister()
    first = _device(a, reg)
    other = _device(b, reg)
    _compare(b, other)
    for cloud in (nc.unclean()["empty"], nc.unclean()["five"]):
        reg.setTarget(cloud)
        v = reg.voxels()
        assert len(v["n"]) == 0 and v["rejected"] == 0
    again = _device(a, reg)
    for k in ("ijk", "n", "mean", "icov"):
        np.testing.assert_array_equal(again[k], first[k])
    assert again["rejected"] == first["rejected"]


def test_a_target_prepared_for_one_scan_is_refused(gpu):
    """pcr_ndt_voxels on a handle whose target scan2Map prepared for that scan's region only refuses with a message (it does not return
    the region's voxels); setTarget makes it answer."""
    room = nc.room()
    scan = room[::3].copy()
    reg = NdtRegister()
    pose = np.eye(4)
    pose[0, 3] = 0.05
    reg.scan2Map(scan, room, pose)
    assert reg.stats()["region_repeats"] == 0
    with pytest.raises(RuntimeError, match="region only.*pcr_set_target"):
        reg.voxels()
    reg.setTarget(room)
    v = reg.voxels()
    o = vr.sort_xyz(oracle.ndt_leaves(room))
    np.testing.assert_array_equal(v["ijk"], o["ijk"][o["n"] > 0])
