"""pcr_backend (simpleslam_amd.pcr.Backend): the back end's key-frame and loop-closure loop in the library, pinned bit for bit to the same
sequence of the public calls that existed before it, written out here (Composed), on a closed drive of 60 key frames whose poses drift."""
import ctypes as C
import math

import numpy as np
import pytest

import global_reloc_scene as grs

pytestmark = pytest.mark.gpu
SC_QUERY, SC_RANK, DISTANCE = 1, 2, 4
N_KF, LAP = 60, 50            # 50 key frames round a block every 4 m, then ten more over the first ten
BATCHES = (0, 25, 50, 55, 60)
BEAMS, AZIMUTHS = 8, 240      # 1 920 points per key frame; dense in azimuth: the walls fix the heading and the position of a revisit
DIST = dict(dist_radius=3.0)  # the drift at the revisit is about 1.3 m: the revisited key frame is in reach, its neighbours 4 m on are not


def course(k):
    """world (x, y, heading) of key frame k: counter-clockwise round the block between the streets x = 100 / 150 and y = 100 / 150"""
    s = (4.0 * k) % 200.0
    leg, t = int(s // 50.0), s % 50.0
    return [(100.0 + t, 100.0, 0.0), (150.0, 100.0 + t, 90.0), (150.0 - t, 150.0, 180.0), (100.0, 150.0 - t, -90.0)][leg]


def drift(k, scale=1.0):
    """what the odometry has accumulated by key frame k: a slow yaw and translation, applied on the map side"""
    a = math.radians(0.02 * k * scale)
    D = np.eye(4)
    D[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    D[:3, 3] = [0.02 * k * scale, -0.012 * k * scale, 0.0]
    return D


def build_scene(beams=BEAMS, azimuths=AZIMUTHS, drift_scale=1.0):
    world, _ = grs.asymmetric_world(300_000, seed=3)
    truth = [grs.planar_pose(world, *course(k)) for k in range(N_KF)]
    scans = [np.ascontiguousarray(grs.scan_at(world, T, seed=500 + k, beams=beams, azimuths=azimuths)) for k, T in enumerate(truth)]
    assert max(len(s) for s in scans) <= 2000
    poses = [drift(k, drift_scale) @ T for k, T in enumerate(truth)]
    # mClosestKfIdx as the front end would record it: the nearest earlier key frame by the (drifted) positions
    pos = np.array([P[:3, 3] for P in poses])
    closest = np.array([-1] + [int(np.argmin(((pos[:i] - pos[i]) ** 2).sum(axis=1))) for i in range(1, N_KF)], np.int64)
    assert (closest[1:LAP - 1] == np.arange(LAP - 2)).all() and (closest[LAP:] < 12).all()      # (the revisit hangs on the first lap)
    return dict(truth=truth, scans=scans, poses=poses, closest=closest)


@pytest.fixture(scope="module")
def scene(gpu):
    return build_scene()


def new_store(scene, upto=0):
    from simpleslam_amd import SubMap
    sm = SubMap()
    for k in range(upto):
        sm.addKeyFrame(scene["scans"][k], scene["poses"][k])
    return sm


def extend(sm, scene, upto):
    for k in range(sm.keyframes(), upto):
        sm.addKeyFrame(scene["scans"][k], scene["poses"][k])


def store_poses(sm):
    return np.array([sm.keyFrame(i)[1] for i in range(sm.keyframes())])


def pose_inv(M):
    """[R^T, -(R^T t)] in the library's order of operations (graph_math.h: pose_inv)"""
    B = np.eye(4)
    for r in range(3):
        for c in range(3):
            B[r, c] = M[c, r]
        B[r, 3] = -((float(M[0, r]) * float(M[0, 3]) + float(M[1, r]) * float(M[1, 3])) + float(M[2, r]) * float(M[2, 3]))
    return B


def pose_mul(A, B):
    """row by row ((a0 b0 + a1 b1) + a2 b2) + t (graph_math.h: pose_mul)"""
    Cm = np.eye(4)
    for c in range(4):
        for r in range(3):
            Cm[r, c] = ((float(A[r, 0]) * float(B[0, c]) + float(A[r, 1]) * float(B[1, c])) + float(A[r, 2]) * float(B[2, c])) + (float(A[r, 3]) if c == 3 else 0.0)
    return Cm


class Composed:
    """The two events from the public calls that existed before pcr_backend, in the order of Backend::optimHandler and
    LoopClosureManager::lcHandler: what a caller had to write."""

    def __init__(self, sm, detectors=SC_QUERY, lc_method="vgicp", grid_size=0.5, context_grid_size=0.5, history_range=1, fitness_threshold=0.3,
                 dist_radius=5.0, lc_between_refined=1):
        from simpleslam_amd import GicpRegister, PoseGraph, ScanContext, VgicpRegister, load_library
        self.lib = load_library()
        self.sm, self.view = sm, sm.view()
        self.sc = ScanContext()
        self.reg = GicpRegister() if lc_method == "gicp" else VgicpRegister()
        self.reg.initForLC()
        self.g = PoseGraph()
        self.p = dict(detectors=detectors, grid_size=grid_size, context_grid_size=context_grid_size, history_range=history_range,
                      fitness_threshold=fitness_threshold, dist_radius=dist_radius, lc_between_refined=lc_between_refined)
        self.done = self.lc_done = 0

    def _finish(self):
        res = self.g.optimize()
        self.g.applyTo(self.sm, 0, self.done)
        return res.delta

    def add_keyframes(self, closest=None):
        n, first = self.sm.keyframes(), self.done
        if n == first:
            return np.eye(4)
        self.sc.addKeyFrames(self.sm, first, n - first, grid_size=self.p["context_grid_size"])      # before saveKfs: the raw key frames
        if self.p["grid_size"] > 0:
            self.sm.downSampleKeyFrames(first, self.p["grid_size"])
        poses = np.array([self.sm.keyFrame(i)[1] for i in range(first, n)])
        if self.g.size() == (0, 0, 0):
            self.g.addPrior(poses[0], id=0)
        self.g.addPoses(poses)
        self.done = n
        for i in range(max(first, 1), n):
            self.g.addOdomFactor(int(closest[i - first]) if closest is not None else i - 1, i)
        return self._finish()

    def close_loops(self):
        first, count = self.lc_done, len(self.sc) - self.lc_done
        self.lc_done = len(self.sc)
        det = self.p["detectors"]
        records = []

        def propose(cur, old, bit, start):
            for r in records[start:]:
                if r["cur"] == cur and r["old"] == old:
                    r["detector"] |= bit
                    return
            records.append(dict(cur=cur, old=old, detector=bit, converged=0, iterations=0, accepted=0, fitness=np.finfo(np.float64).max))

        by_query = [self.sc.query(first + r)[0] for r in range(count)] if det & SC_QUERY else [-1] * count
        by_rank = [m for (_q, m, _y, _d) in self.sc.findLoops(first, count)] if det & SC_RANK and count else [-1] * count
        by_dist = self.view.rankNear(first, count, self.p["dist_radius"], k=1, num_exclude_recent=40)[0][:, 0].tolist() if det & DISTANCE and count else [-1] * count
        for r in range(count):
            start = len(records)
            for old, bit in ((by_query[r], SC_QUERY), (by_rank[r], SC_RANK), (by_dist[r], DISTANCE)):
                if old >= 0:
                    propose(first + r, int(old), bit, start)
        added = 0
        for r in records:
            old_pose = self.sm.keyFrame(r["old"])[1]
            n_sub = self.view.loopFindNearKeyframes(r["old"], self.p["history_range"], self.p["context_grid_size"])
            src, n_cur, _stride = self.sm.keyFramePointer(r["cur"])
            guess = self.sm.keyFrame(r["cur"])[1]
            r["pose"] = guess
            if not src or n_cur == 0 or n_sub == 0:
                continue
            buf = np.ascontiguousarray(guess.T).reshape(-1).copy()
            conv = C.c_int(0)
            assert self.lib.pcr_scan2map_submap(self.reg._h, C.c_void_p(src), n_cur, 1, self.view._m, buf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(conv)) == 0
            r["pose"] = buf.reshape(4, 4).T.copy()
            r["converged"], r["iterations"], r["fitness"] = int(bool(conv.value)), int(self.reg.stats()["iterations"]), self.reg.getFitnessScore()
            if not (r["converged"] and r["fitness"] < self.p["fitness_threshold"]):
                continue
            if self.p["lc_between_refined"]:
                self.g.addLC(r["old"], r["cur"], pose_mul(pose_inv(old_pose), r["pose"]))
            else:
                from simpleslam_amd.pcr import GRAPH_LOOP, graph_noise
                self.g.addOdomFactor(r["old"], r["cur"], info=graph_noise(GRAPH_LOOP))
                self.g.setBetweenRobust(self.g.size()[2] - 1, 1, True)
            r["accepted"] = 1
            added += 1
        return records, (self._finish() if added else np.eye(4))


def contexts(sc):
    return np.array([np.concatenate([a.reshape(-1) for a in sc.descriptor(i)]) for i in range(len(sc))]).reshape(len(sc), -1)


def assert_same_state(be, ref, what):
    np.testing.assert_array_equal(be.graph.poses(), ref.g.poses(), err_msg=f"{what}: graph poses")
    assert be.graph.size() == ref.g.size(), what
    np.testing.assert_array_equal(store_poses(be.map), store_poses(ref.sm), err_msg=f"{what}: store poses")
    np.testing.assert_array_equal(contexts(be.sc), contexts(ref.sc), err_msg=f"{what}: contexts")


def assert_same_records(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        for f in ("cur", "old", "detector", "converged", "iterations", "accepted", "fitness"):
            assert a[f] == b[f], (what, f, a, b)
        np.testing.assert_array_equal(a["pose"], b["pose"], err_msg=what)


def run_library(scene, closest=True, batches=BATCHES, **prm):
    """the whole scene through pcr.Backend in batches -> (backend, per batch: (add info, loop info, records, graph poses, store poses, store poses
    between the two events))"""
    from simpleslam_amd import Backend
    sm = new_store(scene)
    be = Backend(sm, **prm)
    log = []
    for a, b in zip(batches[:-1], batches[1:]):
        extend(sm, scene, b)
        add = be.addKeyFrames(scene["closest"][a:b] if closest else None)
        mid = store_poses(sm)
        lc = be.closeLoops()
        log.append((add, lc, be.loops(), be.graph.poses(), store_poses(sm), mid))
    return be, log


@pytest.mark.parametrize("detectors,lc_method,closest", [(SC_QUERY, "vgicp", True), (SC_RANK, "vgicp", True), (DISTANCE, "vgicp", True),
                                                         (SC_QUERY | SC_RANK | DISTANCE, "vgicp", True), (SC_QUERY | SC_RANK | DISTANCE, "gicp", True),
                                                         (DISTANCE, "vgicp", False), (DISTANCE, "gicp", False)])
def test_every_event_equals_the_composition_of_the_public_calls(scene, detectors, lc_method, closest):
    from simpleslam_amd import Backend
    sm_a, sm_b = new_store(scene), new_store(scene)
    be = Backend(sm_a, detectors=detectors, lc_method=lc_method, **DIST)
    ref = Composed(sm_b, detectors=detectors, lc_method=lc_method, **DIST)
    seen = 0
    for a, b in zip(BATCHES[:-1], BATCHES[1:]):
        extend(sm_a, scene, b)
        extend(sm_b, scene, b)
        cl = scene["closest"][a:b] if closest else None
        info = be.addKeyFrames(cl)
        delta = ref.add_keyframes(cl)
        np.testing.assert_array_equal(info["delta"], delta, err_msg=f"add {a}:{b}: delta")
        assert info["keyframes_added"] == b - a and info["keyframes"] == b and info["contexts"] == b and info["optimized"] == 1
        assert_same_state(be, ref, f"add {a}:{b}")
        info = be.closeLoops()
        records, delta = ref.close_loops()
        assert_same_records(be.loops(), records, f"loops {a}:{b}")
        np.testing.assert_array_equal(info["delta"], delta, err_msg=f"loops {a}:{b}: delta")
        assert info["candidates"] == len(records) and info["accepted"] == sum(r["accepted"] for r in records) == info["factors_added"]
        assert_same_state(be, ref, f"loops {a}:{b}")
        seen += len(records)
    if detectors & DISTANCE:
        assert seen >= 5      # (the revisit is within reach of the distance detector: the comparison covers verified pairs)


def test_contexts_come_from_the_raw_key_frames(scene):
    from simpleslam_amd import Backend, ScanContext
    sm, raw = new_store(scene, 12), new_store(scene, 12)
    be = Backend(sm, grid_size=3.0, context_grid_size=0.5, detectors=0)
    be.addKeyFrames()
    want = ScanContext()
    want.addKeyFrames(raw, 0, 12, grid_size=0.5)
    np.testing.assert_array_equal(contexts(be.sc), contexts(want))
    filtered = ScanContext()
    filtered.addKeyFrames(sm, 0, 12, grid_size=0.5)      # (the store now holds the 3 m key frames: their contexts differ)
    assert not np.array_equal(contexts(filtered), contexts(want))
    assert sm.keyFrame(5)[0].shape[0] < raw.keyFrame(5)[0].shape[0]


def last_error(scene, P):
    return float(np.linalg.norm(P[:3, 3] - scene["truth"][N_KF - 1][:3, 3]))


def test_the_loop_corrects_the_drift(scene):
    """lc_between_refined = 1 (the default): at least one loop is accepted, and the newest key frame lies nearer to its true pose after the
    event that closed it than before."""
    # one event over the whole drive, odometry edges from i - 1: the newest key frame hangs on the chain that the loops pull
    be, log = run_library(scene, closest=False, batches=(0, N_KF), detectors=DISTANCE, **DIST)
    assert sum(lc["accepted"] for _a, lc, _r, _g, _s, _m in log) >= 1
    for k, (_add, lc, _records, _g, after, before) in enumerate(log):
        if lc["accepted"]:
            n = after.shape[0]
            e_before = float(np.linalg.norm(before[n - 1][:3, 3] - scene["truth"][n - 1][:3, 3]))
            e_after = float(np.linalg.norm(after[n - 1][:3, 3] - scene["truth"][n - 1][:3, 3]))
            print(f"batch {k}: {lc['accepted']} loops accepted, newest key frame {e_before:.3f} m -> {e_after:.3f} m from its true pose")
            assert e_after < e_before


def test_the_reference_as_written_corrects_nothing(scene):
    """lc_between_refined = 0: every accepted factor is built from the current estimates, so its residual there is zero to rounding and the
    poses move no further than in a run with no loop factor at all (detectors = 0), which is compared here.  Rounding: a pose coordinate of
    magnitude c carries eps c; a residual built from a handful of such products stays below 64 eps c, and s = r^T Omega r below
    6 * 10 * (64 eps c)^2 under the loop noise's Omega = 10 I."""
    be, log = run_library(scene, closest=False, detectors=DISTANCE, lc_between_refined=0, **DIST)
    none, log0 = run_library(scene, closest=False, detectors=0)
    assert sum(lc["accepted"] for _a, lc, _r, _g, _s, _m in log) >= 1
    injected = np.array(scene["poses"])
    rounding = 64 * np.finfo(np.float64).eps * float(np.abs(injected[:, :3, 3]).max())
    s, _w, robust, _en = be.graph.betweenWeights()
    # (the loop factors stand among the odometry edges, in the order the events added them: they are the marked ones)
    assert robust.sum() == sum(lc["accepted"] for _a, lc, _r, _g, _s, _m in log) and s.size == N_KF - 1 + robust.sum()
    print(f"loop factors' s = r^T Omega r at the final estimate: max {s[robust].max():.3e}; bound {60 * rounding ** 2:.3e}")
    assert s[robust].max() <= 60 * rounding ** 2
    for (_add, _lc, _r, g_poses, _s, _m), (_add0, _lc0, _r0, g0, _s0, _m0) in zip(log, log0):
        moved = float(np.abs(g_poses - injected[:len(g_poses)]).max())
        moved0 = float(np.abs(g0 - injected[:len(g0)]).max())
        print(f"{len(g0)} key frames: moved {moved:.3e} with the reference's loop factors, {moved0:.3e} with none")
        assert moved <= max(moved0, rounding)


def test_a_threshold_of_zero_accepts_nothing(scene):
    be, log = run_library(scene, detectors=DISTANCE, fitness_threshold=0.0, **DIST)
    none, log0 = run_library(scene, detectors=0)
    assert sum(len(r) for _a, _l, r, _g, _s, _m in log) >= 5 and all(lc["accepted"] == 0 and lc["optimized"] == 0 for _a, lc, _r, _g, _s, _m in log)
    assert be.graph.size() == none.graph.size() == (N_KF, 1, N_KF - 1)
    np.testing.assert_array_equal(be.graph.poses(), none.graph.poses())
    np.testing.assert_array_equal(store_poses(be.map), store_poses(none.map))


def snapshot(be):
    return be.graph.poses(), be.graph.size(), contexts(be.sc), store_poses(be.map)


def test_a_bad_closest_entry_changes_nothing_and_reset_starts_over(scene):
    from simpleslam_amd import Backend, PcrError
    sm = new_store(scene, 10)
    be = Backend(sm, detectors=DISTANCE, **DIST)
    first = be.addKeyFrames(scene["closest"][:10])
    extend(sm, scene, 20)
    before = snapshot(be)
    good = scene["closest"][10:20]
    for bad, why in ((np.r_[good[:4], -1, good[5:]], "-1 for a key frame other than 0"), (np.r_[good[:4], 14, good[5:]], "its own index"),
                     (np.r_[good[:4], 17, good[5:]], "beyond its own index"), (np.r_[good[:4], 10 ** 9, good[5:]], "out of range"), (good[:9], "too few entries")):
        with pytest.raises(PcrError):
            be.addKeyFrames(bad)
        for a, b in zip(snapshot(be), before):
            assert np.array_equal(a, b), why
    second = be.addKeyFrames(good)      # (a refused call does not leave the back end failed)
    lc = be.closeLoops()
    after = snapshot(be)
    # reset: the same events on the same key frames give the same bits (the store is the caller's: emptied and filled again here)
    be.reset()
    assert be.graph.size() == (0, 0, 0) and len(be.sc) == 0
    sm.clear()
    extend(sm, scene, 10)
    again_first = be.addKeyFrames(scene["closest"][:10])
    extend(sm, scene, 20)
    again_second = be.addKeyFrames(good)
    again_lc = be.closeLoops()
    np.testing.assert_array_equal(again_first["delta"], first["delta"])
    np.testing.assert_array_equal(again_second["delta"], second["delta"])
    np.testing.assert_array_equal(again_lc["delta"], lc["delta"])
    for a, b in zip(snapshot(be), after):
        np.testing.assert_array_equal(a, b)
    assert lc["contexts"] == 20


def test_two_runs_of_the_whole_scene_give_identical_bits(scene):
    runs = [run_library(scene, detectors=SC_QUERY | SC_RANK | DISTANCE, **DIST) for _ in range(2)]
    for (add_a, lc_a, rec_a, g_a, s_a, _ma), (add_b, lc_b, rec_b, g_b, s_b, _mb) in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(g_a, g_b)
        np.testing.assert_array_equal(s_a, s_b)
        np.testing.assert_array_equal(add_a["delta"], add_b["delta"])
        np.testing.assert_array_equal(lc_a["delta"], lc_b["delta"])
        assert_same_records(rec_a, rec_b, "second run")
    np.testing.assert_array_equal(contexts(runs[0][0].sc), contexts(runs[1][0].sc))


def test_drive_slam_strings_front_end_and_back_end_together(gpu):
    import torch
    from simpleslam_amd import Backend, Frontend, make_register, sequence
    scans, truth, cmds = sequence.make_drive(14, 20261005, map_points=120_000, beams=32, azimuths=512)
    fe = Frontend(make_register("loam"))
    be = Backend(fe.map, detectors=DISTANCE, dist_radius=2.0, dist_exclude_recent=3)
    out = sequence.drive_slam(fe, be, [torch.from_numpy(s).cuda() for s in scans], cmds, truth[0])
    n_poses, n_priors, n_between = be.graph.size()
    closest = fe.closest()
    assert n_poses == out["keyframes"] == fe.map.keyframes() == closest.size >= 3 and n_priors == 1
    assert len(out["events"]) == out["keyframes"]
    # the odometry edges hang where the front end said: one per key frame after the first, in order, from closest[i] to i
    assert n_between >= n_poses - 1
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "slam.g2o")
        be.graph.saveG2o(path)
        edges = [tuple(int(t) for t in line.split()[1:3]) for line in open(path) if line.startswith("EDGE_SE3:QUAT")]
    assert edges[:n_poses - 1] == [(int(closest[i]), i) for i in range(1, n_poses)]
