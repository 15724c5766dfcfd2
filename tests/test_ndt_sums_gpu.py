"""The sums of one NDT pass -- score, gradient, Hessian -- on BOTH families of pass kernels, at the scan sizes where a reduction goes wrong.

  host family     ndt_derivatives_kernel / ndt_hessian_kernel, 128 threads, up to 1024 blocks, folded by ndt_sum_partials_kernel:
                  NdtRegister.derivatives(...) (pcr_ndt_derivatives), the host-driven loop
  device family   ndt_pass_pro_kernel, 512 threads, at most 256 rows, folded in the prologue of the NEXT launch: what scan2Map runs by
                  default.  NdtRegister.derivatives(..., device_loop=True, kind=k) (pcr_ndt_pass_sums) runs that loop's own two
                  launches on a state that asks for one pass and ends; kind 1 is the 7-component pass of the line search, kind 2
                  computeHessian.

Each against oracle.ndt_derivatives at the bars of test_ndt_gpu.py::test_derivatives_match_oracle (1e-9 score, 1e-7 gradient, 1e-8
Hessian, relative to the largest entry), and the two families against each other at the same bars.  The scans are built so that a
dropped lane shows: all points but r (1..3) lie far outside every voxel and add exactly zero, and the r that count sit at the very end
of the scan (the partial last block, the grid-stride round) or at its very start."""
import numpy as np
import pytest

import ndt_clouds as nc
import ndt_voxel_ref as vr
import oracle
from simpleslam_amd import NdtRegister

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 127, 128, 129, 511, 512, 513, 1025]
BIG = 131072 + 513          # the first size at which both families grid-stride (1024 x 128 and 256 x 512 threads) with a ragged tail
P6 = np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.015])


@pytest.fixture(scope="module")
def room_reg(gpu):
    room = nc.room()
    reg = NdtRegister()
    reg.setTarget(room)
    return room, reg


def _scan(n, inside_first):
    """n points: r = 1..3 inside the room (near its floor and walls), the others ~500 m away, where no voxel is"""
    rng = np.random.default_rng(9000 + n)
    r = min(n, 1 + n % 3)
    s = np.zeros((n, 4), np.float32)
    s[:, :3] = 500.0 + rng.uniform(-20, 20, (n, 3))
    inside = np.array([[3.3, 4.6, 0.06], [0.07, 6.4, 1.3], [7.2, 0.05, 2.2]])[:r] + rng.uniform(-0.02, 0.02, (r, 3))
    at = np.arange(r) if inside_first else np.arange(n - r, n)
    if n > 131072:      # the grid-stride size: also the last block and the last row of the first round of either family (256 x 512, 1024 x 128)
        at = np.array([0, 255 * 512 + 7, 1023 * 128 + 5]) if inside_first else np.array([n - 1, 131072 - 1, 250 * 512 + 3])
    s[at, :3] = inside
    return s


def _close(a, b, what):
    """a against b at the bars of test_derivatives_match_oracle"""
    if "score" in a and "score" in b:
        assert abs(a["score"] - b["score"]) <= 1e-9 * abs(b["score"]), (what, a["score"], b["score"])
        assert np.abs(a["grad"] - b["grad"]).max() <= 1e-7 * np.abs(b["grad"]).max(), what
    hs = np.abs(b["hess"]).max() if "hess" in b else None
    if "hess" in a and "hess" in b:
        assert np.abs(a["hess"] - b["hess"]).max() <= 1e-8 * hs, what
    if "hess_d" in a and "hess_d" in b:
        assert np.abs(a["hess_d"] - b["hess_d"]).max() <= 1e-8 * np.abs(b["hess_d"]).max(), what


def _check_both_families(reg, scan, target, p6, what, prm=None):
    o = oracle.ndt_derivatives(scan, target, p6, prm, double_hessian=True)
    assert abs(o["score"]) > 1e-5 and np.abs(o["grad"]).max() > 0 and np.abs(o["hess"]).max() > 0, what      # the points inside count
    host = reg.derivatives(scan, p6, double_hessian=True)
    full = reg.derivatives(scan, p6, device_loop=True, kind=0)
    light = reg.derivatives(scan, p6, device_loop=True, kind=1)
    hd = reg.derivatives(scan, p6, device_loop=True, kind=2)
    assert set(light) == {"score", "grad"}
    for name, got in (("host", host), ("device", full), ("device-7", light), ("device-hessian", hd)):
        _close(got, o, (what, name, "oracle"))
    for name, got in (("device", full), ("device-7", light), ("device-hessian", hd)):
        _close(got, host, (what, name, "host"))
    return o


@pytest.mark.parametrize("inside_first", [False, True], ids=["inside-last", "inside-first"])
@pytest.mark.parametrize("n", SIZES)
def test_ragged_scan_sizes(room_reg, n, inside_first):
    room, reg = room_reg
    _check_both_families(reg, _scan(n, inside_first), room, P6, (n, inside_first))


@pytest.mark.parametrize("inside_first", [False, True], ids=["inside-last", "inside-first"])
def test_grid_stride(room_reg, inside_first):
    room, reg = room_reg
    _check_both_families(reg, _scan(BIG, inside_first), room, P6, (BIG, inside_first))


def test_ordinary_scan(room_reg):
    room, reg = room_reg
    rng = np.random.default_rng(9100)
    scan = room[rng.choice(len(room), 2000, replace=False)].copy()
    scan[:, :3] += rng.normal(0, 0.01, (2000, 3)).astype(np.float32)
    o = _check_both_families(reg, scan, room, P6, "ordinary")
    assert abs(o["score"]) > 100.0


def test_an_empty_scan_sums_to_nothing(room_reg):
    room, reg = room_reg
    for kind in (0, 1, 2):
        d = reg.derivatives(room[:0], P6, device_loop=True, kind=kind)
        assert all(np.all(np.asarray(v) == 0) for v in d.values())


@pytest.mark.parametrize("leaf", nc.FACES_LEAVES)
def test_one_point_scans_a_float_ulp_either_side_of_a_face(gpu, leaf):
    """The lattice is built with floorf(p * inv_leaf) and looked up with floorf(p / leaf) (voxel_grid_covariance_omp_impl.hpp:218-220 and
    :380-382); at these leaves the two disagree at some faces.  The device must look a point up where the oracle does: score and gradient
    of every one-point scan, on both families.

    Tolerance.  The score stays at 1e-9.  The gradient: a wrong voxel changes it by its own size, but the right voxel's icov is the
    oracle's only to the bound of tests/test_ndt_voxels_gpu.py, so its float32 rounding (ndt_omp_impl.hpp:485-537 works in float) may come
    out one ulp apart, and with ONE point nothing averages that out: a gradient entry is e times a sum of three float products, good to a
    few ulps of the largest.  Hence 8 * 2^-24 = 4.8e-7 relative to the largest entry, not the 1e-7 that sums over whole scans meet.  On
    the device one probe of the 288 (leaf 0.3) differs by 2.0e-7 in one gradient entry -- one float ulp of an intermediate -- and every
    other by less than 1e-7."""
    cloud, probes = nc.faces(leaf)
    assert (vr.lattice(probes, leaf)[1][:, 0] != vr.lattice_lookup(probes, leaf)[:, 0]).any()
    reg = NdtRegister(ndt_resolution=leaf)
    reg.setTarget(cloud)
    prm = oracle.ndt_params(resolution=leaf)
    p0 = np.zeros(6)
    tol = 8 * 2.0 ** -24
    hit, worst_s, worst_g = 0, 0.0, 0.0
    for i in range(len(probes)):
        q = probes[i:i + 1]
        o = oracle.ndt_derivatives(q, cloud, p0, prm)
        hit += abs(o["score"]) > 0
        for got in (reg.derivatives(q, p0), reg.derivatives(q, p0, device_loop=True, kind=1)):
            assert abs(got["score"] - o["score"]) <= 1e-9 * abs(o["score"]), (leaf, i, got["score"], o["score"])
            worst_s = max(worst_s, abs(got["score"] - o["score"]) / abs(o["score"]))
            worst_g = max(worst_g, np.abs(got["grad"] - o["grad"]).max() / np.abs(o["grad"]).max())
            assert np.abs(got["grad"] - o["grad"]).max() <= tol * np.abs(o["grad"]).max(), (leaf, i)
    print(f"leaf {leaf}: largest relative difference over the probes: score {worst_s:.2e}, gradient {worst_g:.2e}")
    assert hit == len(probes)


def test_two_complementary_tiles_sum_to_the_untiled_pass(room_reg):
    """NDT's counterpart of test_loam_gpu.py::test_query_tiles_sum_to_the_full_system.  (An NDT handle takes its tile through set_shard --
    voxel-aligned bounds and a halo; set_query_tile serves LOAM handles only.)  Every scan point is evaluated in exactly one tile."""
    room, _ = room_reg
    rng = np.random.default_rng(9200)
    scan = room[rng.choice(len(room), 1500, replace=False)].copy()
    scan[:, :3] += rng.normal(0, 0.01, (1500, 3)).astype(np.float32)
    reg = NdtRegister()
    reg.setTarget(room)
    whole = {dl: reg.derivatives(scan, P6, device_loop=dl) for dl in (False, True)}
    parts = {False: [], True: []}
    for lo, hi in (((-1000.0, -1000.0, -1000.0), (5.0, 1000.0, 1000.0)), ((5.0, -1000.0, -1000.0), (1000.0, 1000.0, 1000.0))):
        reg.set_shard(lo, hi, 1.0)
        reg.setTarget(room)
        for dl in (False, True):
            parts[dl].append(reg.derivatives(scan, P6, device_loop=dl))
    for dl in (False, True):
        a, b = parts[dl]
        assert abs(a["score"]) > 10.0 and abs(b["score"]) > 10.0
        for k in ("score", "grad", "hess"):
            tot, ref = np.asarray(a[k]) + np.asarray(b[k]), np.asarray(whole[dl][k])
            assert np.abs(tot - ref).max() <= 1e-12 * np.abs(ref).max(), (dl, k)
