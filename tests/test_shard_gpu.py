"""The sharded scan2Map (BASELINE configs[3] and the NDT curve of configs[4]) END TO END with more than one rank,
on one card: every rank is a handle of its own (own stream, own tile of the map + halo, one host thread), the exchange of
the normal equations goes through pcr_comm_init_host -- threads of this process (shard.ThreadCollective) or two processes
over gloo.  Between GPUs the same call sequence uses RCCL (pcr_comm_init); no box with more than one GPU was available, so
that transport is covered by the one-rank communicator test in test_loam_gpu.py only.

What must hold (reference loops: PCR/src/LoamRegister.cpp:112-217, ndt_omp_impl.hpp:206-285, fast_vgicp_impl.hpp:119-180):
every rank returns the SAME pose bit for bit (they solve redundantly on identical sums); that pose equals the unsharded HIP
pose up to the order of the additions (<= 1e-12; NDT / VGICP poses leave as Matrix4f: equal, or one float ulp) and the CPU
oracle's within BASELINE's 1e-4."""
import os
import threading

import numpy as np
import pytest

import oracle
from simpleslam_amd import LoamRegister, NdtRegister, VgicpRegister, make_register, pcr, shard, synth

pytestmark = pytest.mark.gpu
S = 20261003 + 4


def run_ranks(method, n_ranks, scan, init, m, resolution=1.0, halo=None, maps=None, via="scan2Map", **kw):
    """n_ranks handles on cuda:0, one host thread each.  -> (poses, converged flags, registers, errors)"""
    import torch
    coll = shard.ThreadCollective(n_ranks, timeout=300.0)
    d_scan = torch.from_numpy(np.ascontiguousarray(scan)).cuda()
    regs, d_tiles, tiles = [], [], []
    for r in range(n_ranks):
        tile = shard.tile_for_method(m, r, n_ranks, method, resolution, halo)
        if maps is not None:
            tile.points = maps[r]
        reg = make_register(method, **kw)
        reg.set_shard(tile.lo, tile.hi, tile.halo)
        reg.comm_init_host(coll.fn(r), r, n_ranks)
        regs.append(reg); tiles.append(tile); d_tiles.append(torch.from_numpy(tile.points).cuda())
    poses, convs, errs = [None] * n_ranks, [None] * n_ranks, [None] * n_ranks

    def work(r):
        pose = init.copy()
        try:
            if via == "scan2Map":
                convs[r] = regs[r].scan2Map(d_scan, d_tiles[r], pose)
            else:
                regs[r].setTarget(d_tiles[r])
                convs[r] = regs[r].align(d_scan, pose)
            poses[r] = pose
        except Exception as e:      # noqa: BLE001  (the test inspects it)
            errs[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(n_ranks)]
    for t in th: t.start()
    for t in th: t.join(600)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    return poses, convs, regs, errs, tiles


def _all_equal(poses):
    for p in poses[1:]:
        np.testing.assert_array_equal(p, poses[0])


@pytest.fixture(scope="module")
def w1m():
    world, m = synth.make_map(1_000_000, seed=S)
    scan, T = synth.make_scan(world, 0, seed=S)
    return dict(map=m, scan=scan, truth=T, init=synth.perturb(T, S))


@pytest.mark.parametrize("n_ranks", [2, 8])
def test_loam_sharded_equals_unsharded(gpu, w1m, n_ranks):
    w = w1m
    kw = dict(loam_iters=10, loam_early_exit=0)
    poses, convs, regs, errs, tiles = run_ranks("loam", n_ranks, w["scan"], w["init"], w["map"], **kw)
    assert errs == [None] * n_ranks, errs
    _all_equal(poses)
    assert len(set(convs)) == 1
    ref = w["init"].copy()
    c_ref = LoamRegister(**kw).scan2Map(w["scan"], w["map"], ref)
    assert convs[0] == c_ref
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 1e-12 and dr <= 1e-12, (dt, dr)
    po, _, _ = oracle.loam_scan2map(w["scan"], w["map"], w["init"], oracle.loam_params(iters=10, early_exit=0, threads=8))
    dt, dr = synth.pose_error(poses[0], po)
    assert dt <= 1e-4 and dr <= 1e-4
    # a tile is what it says: core points balanced, every rank indexed less than the whole map
    assert max(t.points.shape[0] for t in tiles) < 0.75 * w["map"].shape[0]


def test_loam_sharded_reference_defaults_and_static_target(gpu, w1m):
    """8 iterations + early exit (LoamRegister.hpp:37-40): the converged flag and the iteration count come out of the same
    redundantly solved system on every rank; and the prepared-target entry points (pcr_set_target + pcr_align) shard the same way."""
    w = w1m
    ref = w["init"].copy()
    r0 = LoamRegister()
    c_ref = r0.scan2Map(w["scan"], w["map"], ref)
    for via in ("scan2Map", "align"):
        poses, convs, regs, errs, _ = run_ranks("loam", 4, w["scan"], w["init"], w["map"], via=via)
        assert errs == [None] * 4, errs
        _all_equal(poses)
        assert convs == [c_ref] * 4
        assert [r.stats()["iterations"] for r in regs] == [r0.stats()["iterations"]] * 4
        dt, dr = synth.pose_error(poses[0], ref)
        assert dt <= 1e-12 and dr <= 1e-12


def test_config4_ten_iterations_on_a_10m_map_sharded_over_eight_ranks(gpu):
    """BASELINE configs[3] as stated -- pcr=loam, 10 M-point sub-map, 8 ranks, all-reduce of JtJ/JtE per iteration -- end to end."""
    world, m = synth.make_map(10_000_000, seed=S + 2)
    scan, T = synth.make_scan(world, 0, seed=S + 2)
    init = synth.perturb(T, S + 2)
    kw = dict(loam_iters=10, loam_early_exit=0)
    poses, convs, regs, errs, tiles = run_ranks("loam", 8, scan, init, m, **kw)
    assert errs == [None] * 8, errs
    _all_equal(poses)
    assert max(t.points.shape[0] for t in tiles) < 1.35 * 10_000_000 / 8
    ref = init.copy()
    LoamRegister(**kw).scan2Map(scan, m, ref)
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 1e-12 and dr <= 1e-12, (dt, dr)
    po, _, _ = oracle.loam_scan2map(scan, m, init, oracle.loam_params(iters=10, early_exit=0, threads=16))
    dt, dr = synth.pose_error(poses[0], po)
    assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)
    et, er = synth.pose_error(poses[0], T)
    assert et < 0.02 and er < 2e-3


def test_unequal_tiles_one_rank_regrows_its_cell_table(gpu):
    """Quantile-cut slabs of a map of uneven density have unequal boxes: here one tile fits the first-guess cell table
    (2^20 cells) and the other needs three times that.  The rank that must grow and rebuild does so BEFORE the first exchange;
    every rank runs the same number of collectives and none is left waiting (round-1 advisor finding)."""
    world, m = synth.make_map(1_000_000, seed=S)
    scan, T = synth.make_scan(world, 0, seed=S)
    init = synth.perturb(T, S)
    x = m[:, 0]
    x0 = x.min() + 0.2 * (x.max() - x.min())
    rng = np.random.default_rng(7)
    keep = (x < x0) | (rng.random(m.shape[0]) < 0.12)
    m2 = np.ascontiguousarray(m[keep])
    poses, convs, regs, errs, tiles = run_ranks("loam", 2, scan, init, m2)
    assert errs == [None, None], errs

    def cells(t):
        f = np.isfinite(t.points[:, :3]).all(1)
        ext = np.floor(t.points[f, :3].max(0)) - np.floor(t.points[f, :3].min(0)) + 5
        return float(np.prod(ext))
    nc = sorted(cells(t) for t in tiles)
    assert nc[0] < 2 ** 20 < nc[1], nc                      # exactly the situation described above
    _all_equal(poses)
    ref = init.copy()
    c_ref = LoamRegister().scan2Map(scan, m2, ref)
    assert convs == [c_ref, c_ref]
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 1e-12 and dr <= 1e-12


@pytest.fixture(scope="module")
def nd_w():
    world, m = synth.make_map(1_000_000, seed=S + 5, spacing=0.22)
    scan, T = synth.make_scan(world, 0, seed=S + 5, beams=64, azimuths=1024)
    return dict(map=m, scan=scan, truth=T, init=synth.perturb(T, S + 5, trans=0.1, rot_deg=0.5))


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_ndt_sharded_equals_unsharded(gpu, nd_w, n_ranks):
    w = nd_w
    poses, convs, regs, errs, tiles = run_ranks("ndt", n_ranks, w["scan"], w["init"], w["map"], resolution=1.0)
    assert errs == [None] * n_ranks, errs
    _all_equal(poses)
    r0 = NdtRegister()
    ref = w["init"].copy()
    c_ref = r0.scan2Map(w["scan"], w["map"], ref)
    assert convs == [c_ref] * n_ranks
    assert [r.stats()["iterations"] for r in regs] == [r0.stats()["iterations"]] * n_ranks
    # the pose leaves as a Matrix4f (NdtRegister.cpp:28): identical, or one float ulp where the other order of the sums tipped a rounding
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 2e-6 and dr <= 2e-7, (dt, dr)
    po, co, info = oracle.ndt_scan2map(w["scan"], w["map"], w["init"], oracle.ndt_params())
    assert co == convs[0] and info["iterations"] == r0.stats()["iterations"]
    dt, dr = synth.pose_error(poses[0], po)
    assert dt <= 1e-4 and dr <= 1e-4
    assert max(t.points.shape[0] for t in tiles) < 0.75 * w["map"].shape[0]


@pytest.fixture(scope="module")
def vg_w():
    world, m = synth.make_map(400_000, seed=S + 6)
    scan, T = synth.make_scan(world, 0, seed=S + 6)
    return dict(map=m, scan=scan, truth=T, init=synth.perturb(T, S + 6, trans=0.3, rot_deg=2.0))


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_vgicp_sharded_equals_unsharded(gpu, vg_w, n_ranks):
    w = vg_w
    kw = dict(vgicp_resolution=0.5)
    poses, convs, regs, errs, tiles = run_ranks("vgicp", n_ranks, w["scan"], w["init"], w["map"], resolution=0.5, **kw)
    assert errs == [None] * n_ranks, errs
    _all_equal(poses)
    r0 = VgicpRegister(**kw)
    ref = w["init"].copy()
    c_ref = r0.scan2Map(w["scan"], w["map"], ref)
    assert convs == [c_ref] * n_ranks
    assert [r.stats()["iterations"] for r in regs] == [r0.stats()["iterations"]] * n_ranks
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 2e-6 and dr <= 2e-7, (dt, dr)                  # Matrix4f result (VgicpRegister.cpp:37)
    # the fitness score (VgicpRegister.cpp:42-45) is a sum over the ranks' shares of the scan too
    f = [r.getFitnessScore() for r in regs]
    assert len(set(f)) == 1 and abs(f[0] - r0.getFitnessScore()) <= 1e-9 * r0.getFitnessScore()
    po, co, _ = oracle.vgicp_scan2map(w["scan"], w["map"], w["init"], oracle.vgicp_params(resolution=0.5, threads=16))
    assert co == convs[0]
    dt, dr = synth.pose_error(poses[0], po)
    assert dt <= 1e-4 and dr <= 1e-4


def test_vgicp_sharded_with_a_far_outlier_in_the_map(gpu, vg_w):
    """One stray point 20 km away lands in an edge rank's cloud (the outer tiles are open) and makes THAT rank's voxel lattice too large
    for dense tables; the reference's hash map does not care (fast_vgicp_voxel.hpp:129-156).  The rank indexes the bulk of its own cloud,
    as an unsharded handle does (test_vgicp_gpu.py::test_far_outlier_in_the_target): the stray point is in nobody's 20-neighbourhood and
    in no voxel the scan visits, so every rank returns the unsharded pose.  A scan placed AT the stray point reaches the part that was
    left out: the count travels with the ranks' fitness sums and ALL ranks fail the call together (none is left in a collective)."""
    w = vg_w
    kw = dict(vgicp_resolution=0.5)
    m = w["map"].copy()
    m[0, :3] = [2.0e4, -1.0e4, 2857.0]
    poses, convs, regs, errs, tiles = run_ranks("vgicp", 2, w["scan"], w["init"], m, resolution=0.5, **kw)
    assert errs == [None] * 2, errs
    assert max(t.points[:, 0].max() for t in tiles) >= 2.0e4      # the stray point did go to a rank
    _all_equal(poses)
    r0 = VgicpRegister(**kw)
    ref = w["init"].copy()
    c_ref = r0.scan2Map(w["scan"], m, ref)
    assert convs == [c_ref] * 2
    assert [r.stats()["iterations"] for r in regs] == [r0.stats()["iterations"]] * 2
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 2e-6 and dr <= 2e-7, (dt, dr)
    po, co, _ = oracle.vgicp_scan2map(w["scan"], m, w["init"], oracle.vgicp_params(resolution=0.5, threads=16))
    dt, dr = synth.pose_error(poses[0], po)
    assert co == convs[0] and dt <= 1e-4 and dr <= 1e-4
    # the scan moved onto the stray point
    there = w["init"].copy()
    there[:3, 3] += m[0, :3].astype(np.float64) - w["truth"][:3, 3]
    poses, convs, regs, errs, _ = run_ranks("vgicp", 2, w["scan"], there, m, resolution=0.5, **kw)
    assert all(isinstance(e, pcr.PcrError) for e in errs), errs
    assert all("left out" in str(e) for e in errs), errs


def test_vgicp_halo_too_small_fails_on_every_rank(gpu, vg_w):
    """A halo that does not hold the 20 nearest neighbours of the tile's points would change their covariances
    (fast_gicp_impl.hpp:253): the device check finds them, and ALL ranks fail the call together (none is left in a collective)."""
    w = vg_w
    poses, convs, regs, errs, _ = run_ranks("vgicp", 2, w["scan"], w["init"], w["map"], resolution=0.5, halo=0.5, vgicp_resolution=0.5)
    assert all(isinstance(e, pcr.PcrError) for e in errs), errs
    assert any("halo" in str(e) for e in errs)
    assert any("another rank" in str(e) or "halo" in str(e) for e in errs)


def test_a_rank_without_a_usable_target_stops_all_ranks(gpu, w1m):
    """One rank's target cannot be prepared (its cloud is so thin that the 20 nearest neighbours of its tile's points reach past the halo:
    the covariances would not be the whole map's).  The others learn it from the status exchange before the first linearisation and
    return an error instead of waiting for a peer that has left.  A stray point 1e7 m away in one rank's cloud -- a box no dense table can
    hold -- is no such case: LOAM and VGICP index the part of the cloud that matters and succeed on every rank."""
    w = w1m
    n = 3
    stray = np.array([[1.0e7, -1.0e7, 3.0e6, 0.0]], np.float32)

    def maps_for(method, res):
        out = []
        for r in range(n):
            pts = shard.tile_for_method(w["map"], r, n, method, res).points
            out.append(np.ascontiguousarray(np.vstack([pts, stray]) if r == 1 else pts))
        return out
    thin = [shard.tile_for_method(w["map"], r, n, "vgicp", 0.5).points for r in range(n)]
    thin[1] = np.ascontiguousarray(thin[1][::400])
    poses, convs, regs, errs, _ = run_ranks("vgicp", n, w["scan"], w["init"], w["map"], resolution=0.5, maps=thin, vgicp_resolution=0.5)
    assert all(isinstance(e, pcr.PcrError) for e in errs), errs
    assert "another rank" in str(errs[0]) and "another rank" in str(errs[2])
    assert "another rank" not in str(errs[1])
    # VGICP: the rank indexes the bulk of its cloud (the stray point is in nobody's neighbourhood and in no voxel the scan visits)
    poses, convs, regs, errs, _ = run_ranks("vgicp", n, w["scan"], w["init"], w["map"], resolution=0.5, maps=maps_for("vgicp", 0.5), vgicp_resolution=0.5)
    assert errs == [None] * n, errs
    _all_equal(poses)
    ref = w["init"].copy()
    VgicpRegister(vgicp_resolution=0.5).scan2Map(w["scan"], w["map"], ref)
    dt, dr = synth.pose_error(poses[0], ref)
    assert dt <= 2e-6 and dr <= 2e-7, (dt, dr)
    # LOAM indexes a part of such a tile instead -- scan2Map the region around the scan, the prepared-target path (pcr_set_target has no
    # scan to go by) the bulk of the tile -- and succeeds on every rank, with the pose of the unsharded call
    ref = w["init"].copy()
    LoamRegister().scan2Map(w["scan"], w["map"], ref)
    for via in ("scan2Map", "align"):
        poses, convs, regs, errs, _ = run_ranks("loam", n, w["scan"], w["init"], w["map"], maps=maps_for("loam", 1.0), via=via)
        assert errs == [None] * n, (via, errs)
        _all_equal(poses)
        dt, dr = synth.pose_error(poses[0], ref)
        assert dt <= 1e-12 and dr <= 1e-12, (via, dt, dr)


def test_shard_bounds_are_validated(gpu):
    big = shard.BIG
    lo, hi = np.array([-big, -big, -big]), np.array([big, big, big])
    nd = NdtRegister()
    with pytest.raises(pcr.PcrError, match="multiples of ndt_resolution"):
        nd.set_shard(np.array([0.3, -big, -big]), hi, 1.0)
    with pytest.raises(pcr.PcrError, match="halo"):
        nd.set_shard(np.array([2.0, -big, -big]), hi, 0.5)
    nd.set_shard(np.array([2.0, -big, -big]), hi, 1.0)
    with pytest.raises(pcr.PcrError, match="pcr_set_shard"):
        nd.set_query_tile(lo, hi)
    vg = VgicpRegister(vgicp_resolution=0.5)
    with pytest.raises(pcr.PcrError, match="voxel lattice"):
        vg.set_shard(np.array([1.0, -big, -big]), hi, 2.0)
    vg.set_shard(np.array([1.25, -big, -big]), hi, 2.0)
    lm = LoamRegister()
    with pytest.raises(pcr.PcrError, match="gate radius"):
        lm.set_shard(lo, hi, 0.5)
    lm.set_shard(lo, hi, 1.0)


def _proc_worker(rank, world_size, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    world, m = synth.make_map(300_000, seed=S + 8)
    scan, T = synth.make_scan(world, 0, seed=S + 8)
    init = synth.perturb(T, S + 8)
    out = {}
    for method, kw, res in (("loam", dict(loam_iters=10, loam_early_exit=0), 1.0), ("vgicp", dict(vgicp_resolution=0.5), 0.5)):
        tile = shard.tile_for_method(m, rank, world_size, method, res)
        reg = make_register(method, **kw)
        reg.set_shard(tile.lo, tile.hi, tile.halo)
        reg.comm_init_host(shard.gloo_collective(), rank, world_size)
        pose = init.copy()
        conv = reg.scan2Map(torch.from_numpy(scan).cuda(), torch.from_numpy(tile.points).cuda(), pose)
        out[method] = (pose, conv)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_over_gloo(gpu):
    """One process per rank, as on a multi-GPU node (here both on the one card), the exchange on torch.distributed/gloo."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_proc_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    world, m = synth.make_map(300_000, seed=S + 8)
    scan, T = synth.make_scan(world, 0, seed=S + 8)
    init = synth.perturb(T, S + 8)
    for method, kw, tol in (("loam", dict(loam_iters=10, loam_early_exit=0), 1e-12), ("vgicp", dict(vgicp_resolution=0.5), 2e-6)):
        np.testing.assert_array_equal(got[0][method][0], got[1][method][0])
        ref = init.copy()
        c = make_register(method, **kw).scan2Map(scan, m, ref)
        assert got[0][method][1] == c
        dt, dr = synth.pose_error(got[0][method][0], ref)
        assert dt <= tol and dr <= tol, (method, dt, dr)


@pytest.mark.parametrize("method", ["ndt", "vgicp"])
def test_rccl_transport_with_a_one_rank_communicator(gpu, nd_w, vg_w, method):
    """Between GPUs the sums travel through RCCL (pcr_comm_init) instead of the host callback.  No box with two GPUs was available, but a
    communicator of one rank runs the same code -- staging buffer, ncclAllReduce on the handle's stream (SUM for the sums, MAX for the
    'every rank prepared its tile' flag), copy back -- and must leave every number as it was: the host-driven loop of a sharded handle
    then gives the pose of the host-driven loop of an unsharded one, bit for bit."""
    from simpleslam_amd.pcr import default_params
    w = nd_w if method == "ndt" else vg_w
    Reg = NdtRegister if method == "ndt" else VgicpRegister
    kw = {} if method == "ndt" else dict(vgicp_resolution=0.5)
    p_host = default_params(**kw)
    p_host.host_optimiser = 1                                         # NDT: the host-driven loop
    plain, one = Reg(params=p_host), Reg(params=p_host)
    one.comm_init(shard.unique_id(), 0, 1)
    pa, pb = w["init"].copy(), w["init"].copy()
    ca = plain.scan2Map(w["scan"], w["map"], pa)
    cb = one.scan2Map(w["scan"], w["map"], pb)
    assert ca == cb
    np.testing.assert_array_equal(pa, pb)
    assert plain.stats()["iterations"] == one.stats()["iterations"]
    if method == "ndt":
        # with RCCL the sharded NDT loop stays on the device (fold -> ncclAllReduce on the stream -> controller step, in batches):
        # same decisions, the pose within a float ulp of the host-driven loop (elimination instead of the SVD, the device's libm)
        dev = Reg(params=default_params(**kw))
        dev.comm_init(shard.unique_id(), 0, 1)
        pc = w["init"].copy()
        assert dev.scan2Map(w["scan"], w["map"], pc) == ca
        sd, sp = dev.stats(), plain.stats()
        assert (sd["iterations"], sd["kernel_launches"]) == (sp["iterations"], sp["kernel_launches"])
        dt, dr = synth.pose_error(pc, pa)
        assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)
        first = pc.copy()
        for _ in range(5):                                         # batches enqueued beyond the end must not leak into the next call
            pc = w["init"].copy(); dev.scan2Map(w["scan"], w["map"], pc)
            np.testing.assert_array_equal(pc, first)


def _peer_worker(rank, world_size, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    world, m = synth.make_map(300_000, seed=S + 9)
    scan, T = synth.make_scan(world, 0, seed=S + 9)
    init = synth.perturb(T, S + 9)
    tile = shard.tile_for_method(m, rank, world_size, "loam")
    reg = make_register("loam", loam_iters=10, loam_early_exit=0)
    reg.set_shard(tile.lo, tile.hi, tile.halo)
    handles = [None] * world_size
    dist.all_gather_object(handles, reg.comm_peer_export())
    reg.comm_init_peer(handles, rank, world_size)
    info = reg.comm_info()
    d_scan, d_tile = torch.from_numpy(scan).cuda(), torch.from_numpy(tile.points).cuda()
    poses = []
    for _ in range(3):      # (several calls: the sequence numbers and the two parities of the slots keep working)
        pose = init.copy()
        conv = reg.scan2Map(d_scan, d_tile, pose)
        poses.append(pose)
    import time
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(20):
        pose = init.copy(); reg.scan2Map(d_scan, d_tile, pose)
    dt = (time.perf_counter() - t0) / 20
    q.put((rank, dict(poses=poses, conv=conv, info=info, ms=dt * 1e3)))
    dist.barrier()
    dist.destroy_process_group()


def test_peer_exchange_between_two_processes_on_one_card(gpu):
    """pcr_comm_init_peer (prototype): the sums of a sharded LOAM call cross the ranks through receive buffers mapped with hipIpc -- every rank
    pushes its 32 doubles into its slot of every peer's buffer and folds what arrived in rank order, one launch per linearisation, no
    collective library.  Two processes share the one card here (between GPUs the same stores go out over xGMI): both ranks' poses bitwise
    equal, equal to the unsharded pose to rounding, over several calls."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 777) % 2000)
    procs = [ctx.Process(target=_peer_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    world, m = synth.make_map(300_000, seed=S + 9)
    scan, T = synth.make_scan(world, 0, seed=S + 9)
    init = synth.perturb(T, S + 9)
    ref = init.copy()
    c = make_register("loam", loam_iters=10, loam_early_exit=0).scan2Map(scan, m, ref)
    assert got[0]["info"]["transport"] == "peer" and got[0]["info"]["nranks"] == 2 and got[1]["info"]["rank"] == 1
    for k in range(3):
        np.testing.assert_array_equal(got[0]["poses"][k], got[1]["poses"][k])
        np.testing.assert_array_equal(got[0]["poses"][k], got[0]["poses"][0])
    assert got[0]["conv"] == c
    dt, dr = synth.pose_error(got[0]["poses"][0], ref)
    assert dt <= 1e-12 and dr <= 1e-12, (dt, dr)
    print(f"peer exchange, 2 ranks on one card: {got[0]['ms']:.3f} / {got[1]['ms']:.3f} ms per sharded scan2map")


def test_peer_exchange_with_one_rank_runs_the_whole_protocol(gpu):
    """one rank pushing to itself runs the whole protocol (system-scope stores, sequence word, poll, fold): same pose as the unsharded handle
    bit for bit; the per-iteration price of the exchange is printed next to RCCL's one-rank figure (measured on MI355X: 14.4 us against 13.1 us
    -- three dependent trips to fine-grained memory inside one launch cost what RCCL's two launches cost; what the push buys is that its
    length does not grow with the number of ranks)"""
    import time
    import torch
    world, m = synth.make_map(300_000, seed=S + 9)
    scan, T = synth.make_scan(world, 0, seed=S + 9)
    init = synth.perturb(T, S + 9)
    d_scan, d_map = torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda()
    def timed(reg):
        for _ in range(5):
            p = init.copy(); reg.scan2Map(d_scan, d_map, p)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(40):
            p = init.copy(); reg.scan2Map(d_scan, d_map, p)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 40, p
    plain = make_register("loam", loam_iters=10, loam_early_exit=0)
    t_plain, p_plain = timed(plain)
    peer = make_register("loam", loam_iters=10, loam_early_exit=0)
    peer.comm_init_peer([peer.comm_peer_export()], 0, 1)
    t_peer, p_peer = timed(peer)
    rccl = make_register("loam", loam_iters=10, loam_early_exit=0)
    rccl.comm_init(shard.unique_id(), 0, 1)
    t_rccl, p_rccl = timed(rccl)
    np.testing.assert_array_equal(p_peer, p_plain)
    np.testing.assert_array_equal(p_rccl, p_plain)
    print(f"per iteration over the unsharded call: peer exchange {(t_peer - t_plain) * 1e5:.2f} us, reduce + ncclAllReduce {(t_rccl - t_plain) * 1e5:.2f} us")
    assert t_peer < 2.0 * t_rccl, (t_plain, t_peer, t_rccl)


def _peer_worker_ndt(rank, world_size, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    world, m = synth.make_map(300_000, seed=S + 11, spacing=0.3)
    scan, T = synth.make_scan(world, 0, seed=S + 11)
    init = synth.perturb(T, S + 11, trans=0.1, rot_deg=0.5)
    tile = shard.tile_for_method(m, rank, world_size, "ndt")
    reg = make_register("ndt")
    reg.set_shard(tile.lo, tile.hi, tile.halo)
    handles = [None] * world_size
    dist.all_gather_object(handles, reg.comm_peer_export())
    reg.comm_init_peer(handles, rank, world_size)
    d_scan, d_tile = torch.from_numpy(scan).cuda(), torch.from_numpy(tile.points).cuda()
    poses, convs, its = [], [], []
    for _ in range(3):      # (several calls: batches enqueued beyond the end of one call must not leak into the next, the sequence numbers keep agreeing)
        pose = init.copy()
        convs.append(reg.scan2Map(d_scan, d_tile, pose)); poses.append(pose); its.append(reg.stats()["iterations"])
    q.put((rank, dict(poses=poses, conv=convs, iters=its, info=reg.comm_info())))
    dist.barrier()
    dist.destroy_process_group()


def test_ndt_over_the_peer_exchange_between_two_processes_on_one_card(gpu):
    """Sharded NDT with the device-resident loop over the peer exchange (round 5): per evaluation pass the evaluation launch and ONE launch that folds
    this rank's rows, pushes the 48 sums into every peer's receive buffer, folds what arrived in rank order and takes the controller's step
    (ndt.hip: ndt_fold_exchange_ctl_kernel) -- no collective library, no host round trip.  Two processes on the one card: both ranks' poses,
    verdicts and iteration counts equal, bit for bit, over several calls; the pose that of the unsharded handle to rounding."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 1313) % 2000)
    procs = [ctx.Process(target=_peer_worker_ndt, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    world, m = synth.make_map(300_000, seed=S + 11, spacing=0.3)
    scan, T = synth.make_scan(world, 0, seed=S + 11)
    init = synth.perturb(T, S + 11, trans=0.1, rot_deg=0.5)
    ref = init.copy()
    plain = make_register("ndt")
    c = plain.scan2Map(scan, m, ref)
    assert got[0]["info"]["transport"] == "peer" and got[0]["info"]["nranks"] == 2
    for k in range(3):
        np.testing.assert_array_equal(got[0]["poses"][k], got[1]["poses"][k])
        np.testing.assert_array_equal(got[0]["poses"][k], got[0]["poses"][0])
    assert got[0]["conv"] == got[1]["conv"] == [c] * 3
    assert got[0]["iters"] == got[1]["iters"] == [plain.stats()["iterations"]] * 3
    dt, dr = synth.pose_error(got[0]["poses"][0], ref)
    assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)      # (the sums of the sharded loop are added up in another order: a float pose, an ulp or two)


def test_ndt_peer_exchange_with_one_rank_equals_the_rccl_loop(gpu):
    """one rank pushing to itself runs the whole protocol; the sharded device loop over it takes the same passes and arrives at the same pose, bit for
    bit, as the same loop over a one-rank RCCL communicator (same evaluation kernel, same fold order) -- in two launches per pass instead of three
    and a collective.  The price per pass over the unsharded call is printed."""
    import time
    import torch
    world, m = synth.make_map(300_000, seed=S + 11, spacing=0.3)
    scan, T = synth.make_scan(world, 0, seed=S + 11)
    init = synth.perturb(T, S + 11, trans=0.1, rot_deg=0.5)
    d_scan, d_map = torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda()

    def timed(reg):
        for _ in range(5):
            p = init.copy(); reg.scan2Map(d_scan, d_map, p)
        best = float("inf")
        for _ in range(3):          # (the best of three blocks: one slow block -- another tenant of the host, a clock ramp -- must not decide the comparison below)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(30):
                p = init.copy(); reg.scan2Map(d_scan, d_map, p)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 30)
        return best, p, reg.stats()
    plain = make_register("ndt", full_target=1)
    t_plain, p_plain, s_plain = timed(plain)
    peer = make_register("ndt")
    peer.comm_init_peer([peer.comm_peer_export()], 0, 1)
    t_peer, p_peer, s_peer = timed(peer)
    rccl = make_register("ndt")
    rccl.comm_init(shard.unique_id(), 0, 1)
    t_rccl, p_rccl, s_rccl = timed(rccl)
    np.testing.assert_array_equal(p_peer, p_rccl)
    assert s_peer["iterations"] == s_rccl["iterations"] == s_plain["iterations"]
    dt, dr = synth.pose_error(p_peer, p_plain)
    assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)
    passes = max(1, s_rccl["attempts"])
    print(f"sharded NDT, one rank, per call: unsharded {t_plain * 1e3:.3f} ms, peer {t_peer * 1e3:.3f} ms, rccl {t_rccl * 1e3:.3f} ms ({passes} passes)")
    assert t_peer < t_rccl * 1.25, (t_plain, t_peer, t_rccl)          # (bench.py --shard-map measures the price properly; here: not slower than the loop it replaces)


# 129: one past a 128-thread block of ndt_pass_kernel; 513: a multiple of it plus one; 1025: 9 rows, so that a slice of the fold (ndt.hip:
# ndt_fold_rows, 8 loads in flight) has a ragged tail.  tests/test_oracle_vgicp_ndt.py checks on the CPU that the oracle converges from these
# guesses, on Newton systems far from singular, at all three sizes.
@pytest.mark.parametrize("n", [129, 513, 1025])
def test_ndt_sharded_device_loops_on_small_scans(gpu, n):
    """The sharded device loops (ndt_pass_kernel, the fold of its rows, the controller step) over the peer exchange and over RCCL, one rank each, on
    scans of a few blocks: the same pose bit for bit, the same iterations and passes; the iterations of the unsharded loop and its pose to the bar of
    test_ndt_peer_exchange_with_one_rank_equals_the_rccl_loop (float poses whose sums were added in another order)."""
    import torch
    import ndt_clouds as nc
    m, scan, init = nc.room_scan_case(n)
    d_scan, d_map = torch.from_numpy(scan).cuda(), torch.from_numpy(m).cuda()
    plain = make_register("ndt", full_target=1)
    peer = make_register("ndt")
    peer.comm_init_peer([peer.comm_peer_export()], 0, 1)
    rccl = make_register("ndt")
    rccl.comm_init(shard.unique_id(), 0, 1)
    got = {}
    for name, reg in (("plain", plain), ("peer", peer), ("rccl", rccl)):
        p = init.copy()
        conv = reg.scan2Map(d_scan, d_map, p)
        got[name] = (p, conv, reg.stats())
    np.testing.assert_array_equal(got["peer"][0], got["rccl"][0])
    assert got["peer"][1] == got["rccl"][1] == got["plain"][1]
    assert (got["peer"][2]["iterations"], got["peer"][2]["attempts"]) == (got["rccl"][2]["iterations"], got["rccl"][2]["attempts"])
    assert got["peer"][2]["attempts"] > 0                      # (a device loop ran: the host loop reports 0)
    assert got["peer"][2]["iterations"] == got["plain"][2]["iterations"]
    for name in ("peer", "rccl"):
        dt, dr = synth.pose_error(got[name][0], got["plain"][0])
        assert dt <= 2e-6 and dr <= 2e-6, (name, dt, dr)


def _peer_worker_vgicp(rank, world_size, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    world, m = synth.make_map(200_000, seed=S + 12)
    scan, T = synth.make_scan(world, 0, seed=S + 12, beams=32, azimuths=512)
    init = synth.perturb(T, S + 12, trans=0.2, rot_deg=1.0)
    tile = shard.tile_for_method(m, rank, world_size, "vgicp")
    reg = make_register("vgicp")
    reg.set_shard(tile.lo, tile.hi, tile.halo)
    handles = [None] * world_size
    dist.all_gather_object(handles, reg.comm_peer_export())
    reg.comm_init_peer(handles, rank, world_size)
    d_scan, d_tile = torch.from_numpy(scan).cuda(), torch.from_numpy(tile.points).cuda()
    poses, convs, its, fit = [], [], [], []
    for _ in range(3):
        pose = init.copy()
        convs.append(reg.scan2Map(d_scan, d_tile, pose)); poses.append(pose); its.append(reg.stats()["iterations"]); fit.append(reg.getFitnessScore())
    q.put((rank, dict(poses=poses, conv=convs, iters=its, fit=fit, info=reg.comm_info())))
    dist.barrier()
    dist.destroy_process_group()


def test_vgicp_over_the_peer_exchange_between_two_processes_on_one_card(gpu):
    """Sharded VGICP with the device-resident Levenberg-Marquardt loop over the peer exchange (round 5): in front of every pass ONE launch folds this
    rank's rows, pushes the 32 sums into every peer's receive buffer and folds what arrived in rank order (vgicp.hip: vgicp_peer_exchange_kernel);
    the pass's prologue takes the optimiser's step on the result -- no host round trip per pass.  Two processes on the one card: poses, verdicts,
    iteration counts and fitness scores equal on both ranks, bit for bit, over several calls; the pose that of the unsharded handle to a float ulp."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 1717) % 2000)
    procs = [ctx.Process(target=_peer_worker_vgicp, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    world, m = synth.make_map(200_000, seed=S + 12)
    scan, T = synth.make_scan(world, 0, seed=S + 12, beams=32, azimuths=512)
    init = synth.perturb(T, S + 12, trans=0.2, rot_deg=1.0)
    ref = init.copy()
    plain = make_register("vgicp")
    c = plain.scan2Map(scan, m, ref)
    assert got[0]["info"]["transport"] == "peer" and got[0]["info"]["nranks"] == 2
    for k in range(3):
        np.testing.assert_array_equal(got[0]["poses"][k], got[1]["poses"][k])
        np.testing.assert_array_equal(got[0]["poses"][k], got[0]["poses"][0])
    assert got[0]["conv"] == got[1]["conv"] == [c] * 3
    assert got[0]["iters"] == got[1]["iters"] == [plain.stats()["iterations"]] * 3
    assert got[0]["fit"] == got[1]["fit"]
    dt, dr = synth.pose_error(got[0]["poses"][0], ref)
    assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)
