"""The fitness scores on the sparse target index (csrc/sparse_fitness.hip): pcr_fitness, pcr_fitness_gated, pcr_fitness_batch and the scores of
pcr_relocalize on a target whose dense index was cut -- the twins of test_target_cut_to_a_room_gpu.py, two copies of one map 30 km / 20 km / 8 km
apart -- where such a score used to be "the reference's number or a refusal that names the cut".  Now every score is answered: the dense kernel
as ever, and for what it refuses the sparse kernel, which sees every point.  Against brute force (fitness_ref.py over the oracle's float kd-tree):
n_in exact, the score within another summation order's bound.  And because the least float distance of a point is one value whichever index finds
it, and the sparse kernels sum in the dense kernels' order: SPARSE against AUTO bit for bit wherever the dense kernel answers, batch against single
bit for bit whichever kernel answered either.  tests/test_sparse_fitness_host.py holds the same search to its look-up bound on the CPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import fitness_ref as fr
import oracle
import sparse_index_cases as cases
from simpleslam_amd import GicpRegister, LiorfRegister, LoamRegister, NdtRegister, VgicpRegister, synth
from simpleslam_amd.pcr import QUERY_INDEX_SPARSE, PcrError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = fr.DBL_MAX
GATES = (1.0, DBL_MAX)
OFF = np.array([30000.0, 20000.0, 8000.0], np.float32)
I4 = np.eye(4)


@pytest.fixture(scope="module", autouse=True)
def walk_is_bounded_on_the_cpu(tmp_path_factory):
    """No test of this file runs a kernel before the search the kernels compile (csrc/sparse_walk.h under sw::NearestF32) has been held, on the CPU, to
    its look-up bound on the two-cluster cloud, far queries included: a walk whose cost grew with the empty space would hang a GPU."""
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "sparse_index_check")
    assert os.path.exists(exe), "sparse_index_check not built (run __graft_entry__.build())"
    d = tmp_path_factory.mktemp("walk")
    t = cases.two_clusters()
    t.tofile(d / "t.f32"); cases.queries_for(t, seed=11).tofile(d / "q.f32")
    for gate in ("1.0", "3.4028234663852886e+38"):
        out = subprocess.run([exe, "fitness", str(d / "t.f32"), str(d / "q.f32"), gate], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-300:] + out.stderr
        for line in out.stdout.splitlines():
            if line.startswith("q "):
                w = line.split()
                c = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
                assert c["lookups"] <= 102 + 1 + c["box"] * (1 + 5 * c["rows"] + 2 * c["layers"]), line


def _planar(T, dx, dy, yaw_deg):
    """T moved in the map's plane: Rz(yaw) about the sensor, then (dx, dy, 0)"""
    a = math.radians(yaw_deg)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    out = T.copy()
    out[:3, :3] = Rz @ T[:3, :3]
    out[:3, 3] += [dx, dy, 0.0]
    return out


def _ref_d2(src, dst, pose):
    """per-point float squared 1-NN distance of the transformed source; inf where a coordinate is not finite"""
    q = fr.transform_f32(src, pose)
    ok = np.isfinite(q).all(axis=1)
    d2 = np.full(len(q), np.inf, np.float32)
    if ok.any():
        d2[ok] = oracle.knn_f32(dst, q[ok], 1)[1][:, 0]
    return d2


def _assert_ref(got, d2, gate, what):
    s, n = got
    want_s, want_n = fr.gated_from_sq(d2, gate)
    assert n == want_n, (what, n, want_n)
    if want_n == 0:
        assert s == -1.0, (what, s)
    else:
        np.testing.assert_allclose(s, want_s, rtol=fr.sum_order_rtol(want_n), atol=0, err_msg=str(what))


@pytest.fixture(scope="module")
def twins():
    """scene A, and the reference's per-point distances of every pose the tests score, computed once"""
    world, m = synth.make_map(30_000, seed=21)
    scan, T = synth.make_scan(world, 0, seed=21, beams=16, azimuths=512)
    init = synth.perturb(T, 21, trans=0.2, rot_deg=1.0)
    far = m.copy(); far[:, :3] += OFF
    both = np.ascontiguousarray(np.vstack([m, far]))
    there = init.copy(); there[:3, 3] += OFF
    truth_there = T.copy(); truth_there[:3, 3] += OFF
    poses = []
    for k in range(17):      # alternately in the near and the far copy, from 0.1 m / 0.5 degrees off to 1.7 m / 8.5 degrees
        p = synth.perturb(T, 300 + k, trans=0.1 * (k + 1), rot_deg=0.5 * (k + 1))
        if k % 2:
            p[:3, 3] += OFF
        poses.append(p)
    poses = np.array(poses)
    w = dict(map=m, both=both, scan=scan, init=init, truth=T, there=there, truth_there=truth_there, poses=poses)
    w["d2"] = {"near copy": _ref_d2(scan, both, init), "far copy": _ref_d2(scan, both, there)}
    w["poses_d2"] = [_ref_d2(scan, both, p) for p in poses]
    return w


def _make(method, **kw):
    return {"loam": LoamRegister, "ndt": NdtRegister, "vgicp": VgicpRegister, "gicp": GicpRegister, "liorf": LiorfRegister}[method](**kw)


# ---- 1. every score is answered ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_every_score_on_the_twins_is_answered(gpu, twins, method):
    w = twins
    reg = _make(method)
    reg.setTarget(w["both"])
    for gate in GATES:
        kinds = {}
        for where, T in (("near copy", w["init"]), ("far copy", w["there"])):
            assert fr.gated_from_sq(w["d2"][where], gate)[1] > 0
            got = reg.fitnessGated(w["scan"], T, gate)      # (a PcrError here is the parent's refusal)
            _assert_ref(got, w["d2"][where], gate, (method, where, gate))
            info = reg.queryIndexInfo()
            kinds[where] = info["kind"]
            assert info["kind"] in ("dense", "sparse")
            if info["kind"] == "sparse":
                assert info["n_points"] == len(w["both"]) and info["bytes"] == 24 * len(w["both"])
        print(f"{method}, gate {gate:.3g}: answered by {kinds}")
        # the room the dense index was cut to holds one copy at the most: every point of a scan in the other lies beyond a cut face, the dense kernel
        # cannot answer for it, and the answer above came from the sparse index
        assert "sparse" in kinds.values(), kinds


# ---- 2. the batch answers every pose ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_the_batch_answers_every_pose_as_the_single_call_does(gpu, twins, method):
    """1, 8, 9 and 17 poses, the edges of the launch's tiles of 8: under AUTO (the dense kernel, then the sparse one for exactly the poses it refused:
    some of the 17, so that tile sees another count) and under SPARSE (every pose on the sparse kernel: 1, 8, 9 and 17 themselves)"""
    w = twins
    auto, sp = _make(method), _make(method, query_index=QUERY_INDEX_SPARSE)
    auto.setTarget(w["both"]); sp.setTarget(w["both"])
    single = {}
    for K, gate in ((1, 1.0), (8, 1.0), (9, 1.0), (17, 1.0), (17, DBL_MAX), (9, DBL_MAX)):
        s, n = auto.fitnessBatch(w["scan"], w["poses"][:K], gate)
        info = auto.queryIndexInfo()
        assert (n >= 0).all(), (method, K, gate, n)      # no (-1, -1): nothing is refused
        if K > 1:
            assert info["kind"] == "sparse", info         # (poses of both copies: one of them went to the sparse index, and the batch says so)
        s2, n2 = sp.fitnessBatch(w["scan"], w["poses"][:K], gate)
        assert s.tobytes() == s2.tobytes() and n.tobytes() == n2.tobytes(), (method, K, gate)
        assert sp.queryIndexInfo()["kind"] == "sparse"
        for k in range(K):
            if (k, gate) not in single:
                single[(k, gate)] = auto.fitnessGated(w["scan"], w["poses"][k], gate)
                assert single[(k, gate)] == sp.fitnessGated(w["scan"], w["poses"][k], gate), (method, k, gate)
            assert (s[k], int(n[k])) == single[(k, gate)], (method, K, gate, k)
            _assert_ref((s[k], int(n[k])), w["poses_d2"][k], gate, (method, K, gate, k))
    s, n = auto.fitnessBatch(w["scan"], w["poses"], 1.0, 1000)      # a subset of the source: the same two kernels
    s2, n2 = sp.fitnessBatch(w["scan"], w["poses"], 1.0, 1000)
    assert s.tobytes() == s2.tobytes() and n.tobytes() == n2.tobytes() and (n > 0).all()
    idx = (np.arange(1000, dtype=np.int64) * len(w["scan"])) // 1000
    for k in (0, 16):
        _assert_ref((s[k], int(n[k])), w["poses_d2"][k][idx], 1.0, (method, "subset", k))


# ---- 3. relocalisation in the far copy ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_relocalize_in_the_far_copy(gpu, twins, method):
    """from 1 m / 10 degrees off in the copy the room does not cover (on the parent: no hypothesis left to rank, or a refused final score)"""
    w = twins
    reg = _make(method)
    reg.setTarget(w["both"])
    for where, truth in (("far copy", w["truth_there"]), ("near copy", w["truth"])):
        pose = _planar(truth, 0.8, -0.6, 10.0)
        conv, cands, chosen = reg.relocalize(w["scan"], pose)
        et, er = synth.pose_error(pose, truth)
        print(f"{method}, {where}: {len(cands)} candidates, chosen {chosen}: |dt| = {et:.3e} m, |dR| = {er:.3e} rad, score {cands[chosen]['score']:.6g} ({cands[chosen]['n_in']} points)")
        assert et < 0.1, (method, where, et, er)
        assert all(c["n_in"] >= 0 and c["coarse_n_in"] >= 0 for c in cands), cands      # no candidate was refused
        assert (cands[chosen]["score"], cands[chosen]["n_in"]) == reg.fitnessGated(w["scan"], pose, 1.0), (method, where)
        _assert_ref((cands[chosen]["score"], cands[chosen]["n_in"]), _ref_d2(w["scan"], w["both"], pose), 1.0, (method, where))


# ---- 4. sparse equals dense where dense answers ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def compact():
    world, m = synth.make_map(20_000, seed=5)
    scan, T = synth.make_scan(world, 0, seed=5, beams=16, azimuths=256)
    src = scan.copy()
    src[7, 0] = np.nan; src[300, 2] = np.inf
    poses = np.array([synth.perturb(T, 50 + k, trans=0.2 * k, rot_deg=1.0 * k) for k in range(9)])
    return dict(map=m, scan=scan, src=src, truth=T, init=synth.perturb(T, 5, trans=0.2, rot_deg=1.0), poses=poses)


@pytest.mark.parametrize("method", ["loam", "ndt", "vgicp", "gicp", "liorf"])
def test_sparse_is_dense_bit_for_bit_on_a_compact_target(gpu, compact, method):
    w = compact
    auto, sp = _make(method), _make(method, query_index=QUERY_INDEX_SPARSE)
    auto.setTarget(w["map"]); sp.setTarget(w["map"])
    for gate in GATES + (0.05,):
        a, b = auto.fitnessGated(w["src"], w["poses"][1], gate), sp.fitnessGated(w["src"], w["poses"][1], gate)
        assert a == b and a[1] > 0, (method, gate, a, b)
        assert (auto.queryIndexInfo()["kind"], sp.queryIndexInfo()["kind"]) == ("dense", "sparse")
        assert sp.queryIndexInfo()["n_points"] == len(w["map"])
        a, b = auto.fitnessBatch(w["src"], w["poses"], gate), sp.fitnessBatch(w["src"], w["poses"], gate)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (method, gate)
        assert (auto.queryIndexInfo()["kind"], sp.queryIndexInfo()["kind"]) == ("dense", "sparse")
    _assert_ref(sp.fitnessGated(w["src"], w["poses"][1], 1.0), _ref_d2(w["src"], w["map"], w["poses"][1]), 1.0, method)
    pa, pb = w["init"].copy(), w["init"].copy()
    ca, cb = auto.scan2Map(w["scan"], w["map"], pa), sp.scan2Map(w["scan"], w["map"], pb)
    assert ca == cb and pa.tobytes() == pb.tobytes()      # (the setting governs the scores, not the registration)
    fa, fb = auto.getFitnessScore(), sp.getFitnessScore()
    assert fa == fb, (method, fa, fb)
    if method in ("vgicp", "liorf"):      # (the methods that score the scan they kept; the others answer 0, as the reference's do)
        assert fa > 0 and sp.queryIndexInfo()["kind"] == "sparse"


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def handles(gpu, twins):
    """on scene A: AUTO and SPARSE on both copies, and the dense index of the near copy alone"""
    out = dict(auto=LoamRegister(), sparse=LoamRegister(query_index=QUERY_INDEX_SPARSE), near=LoamRegister())
    out["auto"].setTarget(twins["both"]); out["sparse"].setTarget(twins["both"]); out["near"].setTarget(twins["map"])
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_source_sizes_at_the_block_edges(twins, handles, n):
    w = twins
    src = np.ascontiguousarray(w["scan"][:n])
    for where, T in (("near copy", w["init"]), ("far copy", w["there"])):
        for gate in GATES:
            d2 = w["d2"][where][:n]
            a, s = handles["auto"].fitnessGated(src, T, gate), handles["sparse"].fitnessGated(src, T, gate)
            assert a == s, (n, where, gate, a, s)
            _assert_ref(s, d2, gate, (n, where, gate))
    # within the gate of 1 m^2 the far copy, 37 km away, is nobody's neighbour: the score on both copies is the near copy's own, which its dense index
    # answers exactly -- and the sparse kernel sums in the dense kernel's order
    assert handles["sparse"].fitnessGated(src, w["init"], 1.0) == handles["near"].fitnessGated(src, w["init"], 1.0)
    assert handles["near"].queryIndexInfo()["kind"] == "dense"
    b = handles["sparse"].fitnessBatch(src, np.array([w["init"], w["there"]]), 1.0)
    assert (b[0][0], int(b[1][0])) == handles["near"].fitnessGated(src, w["init"], 1.0)


def test_beyond_the_gate_not_finite_on_a_face_and_15_km_away(twins, handles):
    w = twins
    for name in ("auto", "sparse"):
        reg = handles[name]
        # a scan wholly beyond the gate: a value, not an error
        assert reg.fitnessGated(w["scan"], _planar(w["there"], 500.0, 0.0, 0.0), 1.0) == (-1.0, 0), name
        s, n = reg.fitnessBatch(w["scan"], np.array([_planar(w["there"], 500.0, 0.0, 0.0), _planar(w["init"], 0.0, -700.0, 0.0)]), 1.0)
        assert (s == -1.0).all() and (n == 0).all(), name
        # rows that are not finite count for nothing
        src = w["scan"][:600].copy()
        src[3, 1] = np.nan; src[299, 0] = np.inf; src[511, 2] = -np.inf
        for where, T in (("near copy", w["init"]), ("far copy", w["there"])):
            for gate in GATES:
                _assert_ref(reg.fitnessGated(src, T, gate), _ref_d2(src, w["both"], T), gate, (name, "not finite", where, gate))
        # queries on cell faces (whole metres), beside points of either copy
        q = np.zeros((8, 4), np.float32)
        q[:, :3] = np.round(w["both"][[5, 77, 1234, 29_999, 30_005, 31_234, 45_000, 59_999], :3])
        for gate in GATES:
            _assert_ref(reg.fitnessGated(q, I4, gate), fr.nearest_sq(q[:, :3], w["both"])[0], gate, (name, "faces", gate))
        # a source point 15 km from both copies: not counted, and the call returns; ungated it is counted, at its distance
        lone = np.zeros((1, 4), np.float32); lone[0, :3] = (15000.0, 10000.0, 4000.0)
        assert reg.fitnessGated(lone, I4, 1.0) == (-1.0, 0), name
        mixed = np.ascontiguousarray(np.vstack([w["scan"][:300], lone, w["scan"][300:600]]))
        for gate in GATES:
            _assert_ref(reg.fitnessGated(mixed, w["there"], gate), _ref_d2(mixed, w["both"], w["there"]), gate, (name, "15 km", gate))


@pytest.mark.parametrize("n_tgt", [1, 2])
def test_targets_of_one_and_two_points(gpu, n_tgt):
    t = np.zeros((n_tgt, 4), np.float32)
    t[0, :3] = (1.0, -2.0, 0.5)      # (on a cell face)
    if n_tgt == 2:
        t[1, :3] = (30001.25, 19998.0, 8000.5)
    rng = np.random.default_rng(n_tgt)
    src = np.zeros((257, 4), np.float32)
    src[:, :3] = t[rng.integers(0, n_tgt, 257), :3] + rng.normal(0.0, 0.8, (257, 3)).astype(np.float32)
    src[0, :3] = t[0, :3]
    for kw in ({}, dict(query_index=QUERY_INDEX_SPARSE)):
        reg = LoamRegister(**kw)
        reg.setTarget(t)
        for gate in GATES + (0.0,):
            want = fr.fitness_gated(src, t, I4, gate)
            got = reg.fitnessGated(src, I4, gate)
            assert got[1] == want[1] and (want[1] == 0 or abs(got[0] - want[0]) <= fr.sum_order_rtol(want[1]) * want[0]), (n_tgt, kw, gate, got, want)
            b = reg.fitnessBatch(src, np.array([I4, I4]), gate)
            assert (b[0][0], int(b[1][0])) == got and (b[0][1], int(b[1][1])) == got


# ---- 6. refusal without a kept target -----------------------------------------------------------------------------------------------------------

def test_a_callers_device_target_keeps_its_refusal(gpu, twins):
    """pcr_scan2map_device leaves the target in the caller's buffer: the dense index, cut to a room, refuses the copy it does not cover, and the sparse
    index has nothing of the handle's own to be built from -- the refusal stands and says both; setTarget (which copies) answers everything"""
    import torch
    w = twins
    # (a loam handle drops a target it had to cut for one scan; vgicp keeps it, cut.  full_target: no index of the scan's region only, whose
    # refusal is another one)
    reg = VgicpRegister(full_target=1)
    pose = w["there"].copy()
    reg.scan2Map(torch.from_numpy(w["scan"]).cuda(), torch.from_numpy(w["both"]).cuda(), pose)
    got = reg.getFitnessScore()      # the kept scan at the pose found: the dense index's answer, or the refusal
    if got == -1.0:
        msg = reg._lib.pcr_last_error(reg._h).decode()
        assert "cut" in msg and "device buffer of the caller's" in msg, msg
    else:
        np.testing.assert_allclose(got, fr.gated_from_sq(_ref_d2(w["scan"], w["both"], pose), DBL_MAX)[0], rtol=fr.sum_order_rtol(len(w["scan"])), atol=0)
    refused = 0
    for where, T in (("near copy", w["init"]), ("far copy", w["there"])):
        try:
            got = reg.fitnessGated(w["scan"], T, DBL_MAX)
        except PcrError as e:
            assert "cut" in str(e) and "device buffer of the caller's" in str(e), str(e)
            refused += 1
            s, n = reg.fitnessBatch(w["scan"], np.array([T]), DBL_MAX)      # the batch marks the pose, as ever
            assert (s[0], n[0]) == (-1.0, -1)
            continue
        _assert_ref(got, w["d2"][where], DBL_MAX, where)
    assert refused >= 1, "a room that covers both copies?"
    reg.set_params(query_index=QUERY_INDEX_SPARSE)
    with pytest.raises(PcrError, match="device buffer of the caller's"):
        reg.fitnessGated(w["scan"], w["init"], 1.0)
    reg.set_params(query_index=0)
    reg.setTarget(torch.from_numpy(w["both"]).cuda())      # (copied: the handle's own from now on)
    for where, T in (("near copy", w["init"]), ("far copy", w["there"])):
        _assert_ref(reg.fitnessGated(w["scan"], T, DBL_MAX), w["d2"][where], DBL_MAX, ("after setTarget", where))


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------------------

def test_two_identical_calls_return_identical_bytes(twins, handles):
    w = twins
    for name in ("auto", "sparse"):
        reg = handles[name]
        for gate in GATES:
            assert reg.fitnessGated(w["scan"], w["there"], gate) == reg.fitnessGated(w["scan"], w["there"], gate)
            a, b = reg.fitnessBatch(w["scan"], w["poses"], gate), reg.fitnessBatch(w["scan"], w["poses"], gate)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
