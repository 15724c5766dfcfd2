"""Global relocalisation on the device: pcr_sc_distances (sc_rank_kernel) against the host's pcr_sc_distance bit for bit, and
pcr_relocalize_global end to end with no prior, on a synthetic city whose buildings no longer repeat (tests/global_reloc_scene.py)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import global_reloc_scene as gs
import oracle
from simpleslam_amd import LoamRegister, ScanContext, VgicpRegister, global_reloc_hypotheses, global_reloc_params, synth
from simpleslam_amd.pcr import GlobalRelocCandidate, PcrError
from test_scancontext_gpu import _scan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(autouse=True)
def _need_gpu(gpu):
    return gpu


def _rotated(c, deg):
    th = np.deg2rad(deg)
    r = c.copy()
    r[:, 0] = np.cos(th) * c[:, 0] - np.sin(th) * c[:, 1]
    r[:, 1] = np.sin(th) * c[:, 0] + np.cos(th) * c[:, 1]
    return r


def _edge():
    """points on ring and sector edges (test_scancontext_gpu's construction)"""
    edge = np.zeros((64, 8), np.float32)
    edge[:20, 0] = np.arange(1, 21) * 4.0
    edge[20:40, 1] = -np.arange(1, 21) * 4.0
    edge[40:50, 0] = -np.arange(1, 11) * 7.0
    edge[50:60, 0] = -np.arange(1, 11) * 7.0
    edge[50:60, 1] = -0.0
    edge[60] = 0
    edge[61, :3] = [80.0, 0, 1]
    edge[62, :3] = [56.568542, 56.568542, 1]
    edge[63, :3] = [0.0, -80.0, 1]
    edge[:, 2] += np.linspace(-3, 3, 64, dtype=np.float32)
    return edge


def _assert_like_host(sc, cloud, dist, shift):
    """(dist, shift) from pcr_sc_distances == pcr_sc_distance(q, i) once the cloud is added as context q (which it then stays)"""
    q = len(sc)
    sc.addContext(cloud)
    for i in range(q):
        assert (dist[i], shift[i]) == sc.distance(q, i), (i, dist[i], shift[i], sc.distance(q, i))


def test_distances_equal_the_host_distance():
    base = _scan(7, n=20000, reach=70.0)
    clouds = [_scan(1), _scan(2, n=100), _scan(3, reach=20.0), np.zeros((0, 8), np.float32), _edge()]
    clouds += [_rotated(base, 6.0 * k) for k in (0, 7, 31, 59)] + [_rotated(base, 100.0)]
    queries = [_rotated(base, 6.0 * 12), _edge(), _scan(1), np.zeros((0, 8), np.float32), _rotated(_scan(9, n=3000), 17.0)]
    for qc in queries:
        sc, orc = ScanContext(), oracle.ScanContextOracle()
        for c in clouds:
            sc.addContext(c)
            orc.add(c)
        dist, shift = sc.distances(qc)
        assert dist.dtype == np.float64 and shift.dtype == np.int32 and len(dist) == len(clouds)
        assert (dist[3], shift[3]) == (DBL_MAX, 0)                     # the empty context
        if len(qc) == 0:
            assert (dist == DBL_MAX).all() and (shift == 0).all()
        _assert_like_host(sc, qc, dist, shift)
        orc.add(qc)
        for i in range(len(clouds)):
            do, so = orc.distance(len(clouds), i)
            assert so == shift[i] and (abs(dist[i] - do) < 1e-12 or dist[i] == do), (i, dist[i], do)
    d, s = ScanContext().distances(_scan(1))                          # an empty database
    assert d.shape == (0,) and s.shape == (0,)


def test_twenty_thousand_contexts_equal_the_host_loop():
    rng = np.random.default_rng(3)
    sc = ScanContext()
    M = 20_000
    twin = _scan(77, n=400, reach=85.0)
    for i in range(M):
        if i in (5, 12_345):
            sc.addContext(twin)
            continue
        n = 150
        c = np.zeros((n, 4), np.float32)
        r = rng.uniform(1.0, 85.0, n); a = rng.uniform(-np.pi, np.pi, n)
        c[:, 0], c[:, 1], c[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 10.0, n)
        sc.addContext(c)
    assert len(sc) == M
    dist, shift = sc.distances(twin)
    assert dist[5] == dist[12_345] and shift[5] == shift[12_345] == 0 and dist[5] < 1e-12
    order = np.lexsort((np.arange(M), dist))
    assert list(order[:2]) == [5, 12_345]
    _assert_like_host(sc, twin, dist, shift)
    d2, s2 = sc.distances(twin)                                        # one more context now: the same for the others
    assert d2[:M].tobytes() == dist.tobytes() and s2[:M].tobytes() == shift.tobytes()


def test_sources_and_strides_agree_and_the_database_is_unchanged():
    import torch
    prm = dict(num_exclude_recent=3, build_tree_gap=2, num_candidates=3)
    a, b = ScanContext(**prm), ScanContext(**prm)
    clouds = [_rotated(_scan(20 + i, n=2000), 6.0 * i) for i in range(10)]
    q = _scan(21, n=5000)
    qs = [np.ascontiguousarray(q[:, :width]) for width in (3, 4, 8)]     # strides 12, 16, 32 B
    for i, c in enumerate(clouds):
        a.addContext(c)
        b.addContext(c)
        if i < 4:
            continue
        want = a.distances(qs[0])
        for qq in qs:
            for src in (qq, torch.from_numpy(qq).cuda()):
                got = a.distances(src)
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert len(a) == i + 1
        assert a.query(i) == b.query(i), i
        for j in range(i):
            assert a.distance(i, j) == b.distance(i, j)
        assert np.array_equal(a.descriptor(i)[0], b.descriptor(i)[0])


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    world, m = gs.asymmetric_world(300_000, seed=7)
    kf = gs.drive_poses(world)
    kf_scans = [gs.scan_at(world, T, seed=1000 + i) for i, T in enumerate(kf)]
    qp = gs.query_poses(world)
    q_scans = [gs.scan_at(world, T, seed=50 + i) for i, T in enumerate(qp)]
    sc = ScanContext()
    for s in kf_scans:
        sc.addContext(s)
    return dict(world=world, map=m, kf=kf, kf_scans=kf_scans, queries=qp, q_scans=q_scans, sc=sc)


def _yaw(T):
    return math.atan2(T[1, 0], T[0, 0])


def _ang(a):
    return abs((a + math.pi) % (2 * math.pi) - math.pi)


def test_coarse_pose_sign(scene):
    """a key frame's own scan seen after the sensor turned: its points rotated by +theta are what a sensor turned by -theta sees.  The
    coarse pose of the place is within one sector of that truth, and the opposite sign is not."""
    k = 40
    T = scene["kf"][k]
    sc = ScanContext()
    sc.addContext(scene["kf_scans"][k])
    for theta in (80.0, 200.0, -37.0):
        d, s = sc.distances(_rotated(scene["kf_scans"][k], theta))
        truth = T.copy()
        a = math.radians(-theta)
        truth[:3, :3] = T[:3, :3] @ np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        coarse = global_reloc_hypotheses(T, int(s[0]), xy_range=0.0, yaw_range=0.0)[0]
        assert _ang(_yaw(coarse) - _yaw(truth)) <= math.radians(6.0), (theta, s[0], math.degrees(_yaw(coarse)), math.degrees(_yaw(truth)))
        flipped = global_reloc_hypotheses(T, -int(s[0]), xy_range=0.0, yaw_range=0.0)[0]
        assert _ang(_yaw(flipped) - _yaw(truth)) > math.radians(30.0)
        np.testing.assert_array_equal(coarse[:3, 3], T[:3, 3])


METHODS = {"loam": LoamRegister, "vgicp": VgicpRegister}


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_relocalize_global_end_to_end(scene, method):
    """NDT is not covered: on this scene's 0.2 m map it ended 0.13 m from the truth for the first query, and an align from the true pose
    ends 0.14 m from that again -- NDT's own minima on these planar streets, not a property of the global search"""
    reg = METHODS[method]()
    reg.setTarget(scene["map"])
    for q, (scan, T) in enumerate(zip(scene["q_scans"], scene["queries"])):
        dist, _ = scene["sc"].distances(scan)
        top = int(np.lexsort((np.arange(len(dist)), dist))[0])
        assert np.linalg.norm(scene["kf"][top][:2, 3] - T[:2, 3]) < 5.0, (q, top)
        pose = np.eye(4)
        conv, cands, chosen = reg.relocalizeGlobal(scan, scene["sc"], scene["kf"], pose)
        et, er = synth.pose_error(pose, T)
        assert et <= 0.05 and er <= math.radians(0.5), (method, q, et, math.degrees(er), [(c["place"], c["n_in"], c["score"]) for c in cands])
        np.testing.assert_array_equal(pose, cands[chosen]["pose"])
        assert conv == cands[chosen]["converged"]
        assert cands[0]["place"] == top
        places = [c["place"] for c in cands]
        assert places == sorted(places, key=lambda p: (dist[p], p))      # by place rank


def test_candidates_are_align_from_their_hypothesis_and_calls_repeat(scene):
    sc, kf, m = scene["sc"], scene["kf"], scene["map"]
    scan = scene["q_scans"][1]
    reg = VgicpRegister()
    reg.setTarget(m)
    pose = np.eye(4)
    _, cands, chosen = reg.relocalizeGlobal(scan, sc, kf, pose)
    got = reg.getFitnessScore()
    pose2 = np.eye(4)
    _, cands2, chosen2 = reg.relocalizeGlobal(scan, sc, kf, pose2)
    assert pose.tobytes() == pose2.tobytes() and chosen == chosen2
    assert [(c["place"], c["hypothesis"], c["pose"].tobytes(), c["n_in"], c["score"]) for c in cands] == \
           [(c["place"], c["hypothesis"], c["pose"].tobytes(), c["n_in"], c["score"]) for c in cands2]
    fresh = VgicpRegister()
    fresh.setTarget(m)
    for c in cands:
        assert c["sc_shift"] == sc.distances(scan)[1][c["place"]]
        p = global_reloc_hypotheses(kf[c["place"]], c["sc_shift"])[c["hypothesis"]].copy()
        assert fresh.align(scan, p) == c["converged"]
        np.testing.assert_array_equal(p, c["pose"])
    fs, fn = reg.fitnessBatch(scan, np.array([c["pose"] for c in cands]), 1.0, 0)
    assert [(c["score"], c["n_in"]) for c in cands] == list(zip(fs, fn))
    # getFitnessScore afterwards: the chosen pose's (a fresh align from the chosen hypothesis)
    c = cands[chosen]
    again = VgicpRegister()
    again.setTarget(m)
    p = global_reloc_hypotheses(kf[c["place"]], c["sc_shift"])[c["hypothesis"]].copy()
    again.align(scan, p)
    assert got == again.getFitnessScore()


def test_refusals(scene):
    sc, kf, m = scene["sc"], scene["kf"], scene["map"]
    scan = scene["q_scans"][0]
    reg = LoamRegister()
    reg.setTarget(m)
    pose = np.eye(4)
    stranger = _scan(4242, n=20000)
    with pytest.raises(PcrError, match="no place qualifies"):
        reg.relocalizeGlobal(stranger, sc, kf, pose, max_dist=1e-3)
    np.testing.assert_array_equal(pose, np.eye(4))
    with pytest.raises(PcrError, match="n_kf"):
        reg.relocalizeGlobal(scan, sc, kf[:-1], pose)
    reg.relocalizeGlobal(scan, sc, kf, pose)                           # usable afterwards
    assert synth.pose_error(pose, scene["queries"][0])[0] < 0.05
    # capacity below places x refine_top
    p = global_reloc_params()
    kf_cm = np.ascontiguousarray(kf.transpose(0, 2, 1)).reshape(-1)
    cands = (GlobalRelocCandidate * 16)()
    out = np.zeros(16)
    dp = ctypes.POINTER(ctypes.c_double)
    conv, nc, ch = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = reg._lib.pcr_relocalize_global(reg._h, sc._s, kf_cm.ctypes.data_as(dp), len(kf), scan.ctypes.data_as(ctypes.c_void_p), len(scan), 16, 0,
                                        ctypes.byref(p), out.ctypes.data_as(dp), ctypes.byref(conv), cands, 9, ctypes.byref(nc), ctypes.byref(ch))
    assert rc != 0 and "places x refine_top = 10" in reg._lib.pcr_last_error(reg._h).decode()
    # tiled and sharded handles
    reg.set_query_tile([-1e9] * 3, [1e9] * 3)
    with pytest.raises(PcrError, match="query tile"):
        reg.relocalizeGlobal(scan, sc, kf, pose)
    sharded = LoamRegister()
    sharded.setTarget(m)
    sharded.comm_init_host(lambda ptr, count, op, user: 0, 0, 1)
    with pytest.raises(PcrError, match="sharded"):
        sharded.relocalizeGlobal(scan, sc, kf, pose)


CPP = r'''
#include <cstdio>
#include <fstream>
#include <vector>
#include "PCR/HipRegister.hpp"

static std::vector<float> load(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<float> v((size_t)f.tellg() / 4);
    f.seekg(0);
    f.read((char*)v.data(), v.size() * 4);
    return v;
}
static PCR::PC_Ptr cloud(const std::vector<float>& v, size_t off, size_t n) {
    auto pc = std::make_shared<PCR::PointCloud>();
    pc->points.resize(n);
    for (size_t i = 0; i < n; ++i) {
        auto& p = pc->points[i];
        p.x = v[(off + i) * 4]; p.y = v[(off + i) * 4 + 1]; p.z = v[(off + i) * 4 + 2]; p.intensity = v[(off + i) * 4 + 3];
    }
    return pc;
}
int main(int argc, char** argv) {
    const std::vector<float> map = load(argv[1]), kfs = load(argv[2]), scan = load(argv[3]);
    std::ifstream pf(argv[4], std::ios::binary | std::ios::ate);
    std::vector<PCR::pose_t> poses((size_t)pf.tellg() / sizeof(PCR::pose_t));
    pf.seekg(0);
    pf.read((char*)poses.data(), poses.size() * sizeof(PCR::pose_t));
    const size_t per = kfs.size() / 4 / poses.size();
    context::ScanContext sc;
    for (size_t k = 0; k < poses.size(); ++k) sc.addContext(*cloud(kfs, k * per, per));
    auto reg = PCR::makeStaticMapRegister("loam");
    PCR::pose_t res;
    std::vector<pcr_global_reloc_candidate> cands;
    size_t chosen = 0;
    const bool ok = reg->relocalizeGlobal(cloud(scan, 0, scan.size() / 4), cloud(map, 0, map.size() / 4), sc, poses, res, nullptr, &cands, &chosen);
    if (!ok && !reg->lastError().empty()) { std::fprintf(stderr, "%s\n", reg->lastError().c_str()); return 1; }
    std::printf("chosen %zu place %lld of %zu\n", chosen, (long long)cands[chosen].place, cands.size());
    for (int r = 0; r < 4; ++r) std::printf("%.17g %.17g %.17g %.17g\n", res(r, 0), res(r, 1), res(r, 2), res(r, 3));
    return 0;
}
'''


def test_cpp_mirror_prints_the_python_pose(scene, tmp_path):
    """StaticMapRegister::relocalizeGlobal (host/PCR/HipRegister.hpp, 32-byte PointXYZI records) gives the Python call's pose bit for bit"""
    (tmp_path / "main.cpp").write_text(CPP)
    lib = os.path.join(ROOT, "simpleslam_amd", "lib")
    exe = tmp_path / "global_reloc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simpleslam_amd", "host"), str(tmp_path / "main.cpp"), "-o", str(exe),
                    "-L", lib, "-lpcr_hip", f"-Wl,-rpath,{lib}"], check=True, timeout=300)
    kf = scene["kf"]
    scene["map"].tofile(tmp_path / "map.bin")
    np.concatenate(scene["kf_scans"]).tofile(tmp_path / "kf.bin")
    scan = scene["q_scans"][2]
    scan.tofile(tmp_path / "scan.bin")
    np.ascontiguousarray(kf.transpose(0, 2, 1)).tofile(tmp_path / "poses.bin")
    out = subprocess.run([str(exe), str(tmp_path / "map.bin"), str(tmp_path / "kf.bin"), str(tmp_path / "scan.bin"), str(tmp_path / "poses.bin")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    reg = LoamRegister()
    reg.setTarget(scene["map"])
    pose = np.eye(4)
    _, cands, chosen = reg.relocalizeGlobal(scan, scene["sc"], kf, pose)
    assert lines[0] == f"chosen {chosen} place {cands[chosen]['place']} of {len(cands)}", lines[0]
    assert lines[-4:] == [" ".join(f"{v:.17g}" for v in row) for row in pose]
    assert synth.pose_error(pose, scene["queries"][2])[0] < 0.05
