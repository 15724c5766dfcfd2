"""A session to disk and back on the GPU: pcr_map_save / pcr_map_load on a store whose key-frame sizes sit at the copy's and the filter's
edges, and pcr_backend_set_save_dir / _save / _load pinned bit for bit to the same load written out in public calls -- then a second
session that closes a loop onto a key frame of the first, which no call could do before a session could be loaded."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import session_ref as sr
import session_scene as ss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SPLIT = ss.N_KF, ss.SPLIT


def key_frames(sm):
    return [sm.keyFrame(i) for i in range(sm.keyframes())]


def assert_same_store(a, b, what):
    ka, kb = key_frames(a), key_frames(b)
    assert len(ka) == len(kb), what
    for i, ((ca, pa), (cb, pb)) in enumerate(zip(ka, kb)):
        assert ca.shape == cb.shape and ca.tobytes() == cb.tobytes(), f"{what}: key frame {i}"
        assert pa.tobytes() == pb.tobytes(), f"{what}: pose {i}"


# ---- the store ----
@pytest.fixture(scope="module")
def saved_store(gpu, tmp_path_factory):
    from simpleslam_amd import SubMap
    clouds, poses, stamps = ss.store_scene()
    sm = SubMap()
    for c, T in zip(clouds, poses):
        sm.addKeyFrame(c, T)
    d = str(tmp_path_factory.mktemp("store"))
    sm.save(d, stamps=stamps)
    return dict(sm=sm, dir=d, clouds=clouds, poses=poses, stamps=stamps)


def test_store_save_then_load_gives_the_bytes_back(saved_store):
    from simpleslam_amd import SubMap
    s = saved_store
    assert sorted(os.listdir(s["dir"])) == ["0.pcd", "1.pcd", "2.pcd", "3.pcd", "4.pcd", "tum.txt"]
    want_stamps, want_poses = sr.load_tum(os.path.join(s["dir"], "tum.txt"))
    assert open(os.path.join(s["dir"], "tum.txt")).read() == "".join(sr.tum_format(t, T) for t, T in zip(s["stamps"], s["poses"]))
    sm = SubMap()
    stamps = sm.load(s["dir"])
    assert stamps.tobytes() == want_stamps.tobytes() and sm.keyframes() == 5
    for i, (c, T) in enumerate(key_frames(sm)):
        assert c.shape == s["clouds"][i].shape and c.tobytes() == s["clouds"][i].tobytes(), i
        assert T.tobytes() == want_poses[i].tobytes(), i
        assert np.abs(T[:3, 3] - s["poses"][i][:3, 3]).max() <= 5e-4 + 1e-12      # the default format's own bound
    # precise: the translations come back bit for bit
    sm.save(s["dir"], stamps=s["stamps"], precise=True)
    again = SubMap()
    again.load(s["dir"])
    # (the store was itself loaded from six-digit quaternions: what is compared is what it held)
    for (c, T), (c2, T2) in zip(key_frames(sm), key_frames(again)):
        assert c.tobytes() == c2.tobytes() and T[:3, 3].tobytes() == T2[:3, 3].tobytes()
    saved_store["sm"].save(s["dir"], stamps=s["stamps"])      # (the module's files as they were)


def test_store_load_with_a_grid_equals_the_filter_on_a_store_built_by_hand(saved_store):
    from simpleslam_amd import SubMap
    s = saved_store
    loaded = SubMap()
    loaded.load(s["dir"], grid_size=0.5)
    _stamps, poses = sr.load_tum(os.path.join(s["dir"], "tum.txt"))
    hand = SubMap()
    for i in range(5):
        hand.addKeyFrame(ss.pcd_body(os.path.join(s["dir"], f"{i}.pcd")), poses[i])
    hand.downSampleKeyFrames(0, 0.5)
    assert_same_store(loaded, hand, "grid 0.5")
    assert loaded.keyFrame(4)[0].shape[0] < 300 and loaded.keyFrame(0)[0].shape[0] == 0 and loaded.keyFrame(1)[0].shape[0] == 1


def test_store_save_from_a_view_and_from_first(saved_store, tmp_path):
    s = saved_store
    (tmp_path / "view").mkdir()
    view = s["sm"].view()
    view.updateAll(0.5)
    view.save(str(tmp_path / "view"), stamps=s["stamps"])
    for f in sorted(os.listdir(s["dir"])):
        assert open(tmp_path / "view" / f, "rb").read() == open(os.path.join(s["dir"], f), "rb").read(), f
    (tmp_path / "tail").mkdir()
    s["sm"].save(str(tmp_path / "tail"), first=3, stamps=s["stamps"])
    assert sorted(os.listdir(tmp_path / "tail")) == ["3.pcd", "4.pcd", "tum.txt"]
    assert len(open(tmp_path / "tail" / "tum.txt").read().splitlines()) == 5
    assert open(tmp_path / "tail" / "tum.txt").read() == open(os.path.join(s["dir"], "tum.txt")).read()
    s["sm"].save(str(tmp_path / "tail"))      # stamps None: the key frame's index
    assert [ln.split()[0] for ln in open(tmp_path / "tail" / "tum.txt").read().splitlines()] == ["0.000", "1.000", "2.000", "3.000", "4.000"]


def test_store_load_refusals_leave_the_store_empty(saved_store, tmp_path):
    from simpleslam_amd import PcrError, SubMap
    s = saved_store
    full = SubMap()
    full.addKeyFrame(s["clouds"][2], s["poses"][2])
    with pytest.raises(PcrError, match="holds 1 key frames"):
        full.load(s["dir"])
    assert full.keyframes() == 1 and full.keyFrame(0)[0].tobytes() == s["clouds"][2].tobytes()
    sm = SubMap()
    missing = tmp_path / "missing"
    shutil.copytree(s["dir"], missing)
    os.remove(missing / "2.pcd")
    with pytest.raises(PcrError, match="2.pcd"):
        sm.load(str(missing))
    assert sm.keyframes() == 0
    bad = tmp_path / "bad"
    shutil.copytree(s["dir"], bad)
    lines = open(bad / "tum.txt").read().splitlines()
    lines[1] = " ".join(lines[1].split()[:7])      # line 2, seven numbers
    (bad / "tum.txt").write_text("\n".join(lines) + "\n")
    with pytest.raises(PcrError, match="tum.txt line 2"):
        sm.load(str(bad))
    assert sm.keyframes() == 0
    # no tum.txt: nothing loaded, no error (the reference warns and starts fresh); a blank line is skipped, not counted
    (tmp_path / "empty").mkdir()
    assert sm.load(str(tmp_path / "empty")).size == 0 and sm.keyframes() == 0
    lines = open(os.path.join(s["dir"], "tum.txt")).read().splitlines()
    (missing / "tum.txt").write_text(lines[0] + "\n\n" + lines[1] + "\n   \n")
    assert sm.load(str(missing)).size == 2 and sm.keyframes() == 2      # (0.pcd and 1.pcd: the missing 2.pcd is not asked for)


# ---- the back end ----
@pytest.fixture(scope="module")
def drive(gpu):
    return ss.build_drive()


def new_store(drive, lo=0, hi=0, sm=None):
    from simpleslam_amd import SubMap
    sm = sm or SubMap()
    for k in range(lo, hi):
        sm.addKeyFrame(drive["scans"][k], drive["poses"][k])
    return sm


@pytest.fixture(scope="module")
def session_a(drive, tmp_path_factory):
    """session A: key frames 0:8 in two events with a save directory, then pcr_backend_save"""
    from simpleslam_amd import Backend
    d = str(tmp_path_factory.mktemp("session_a"))
    sm = new_store(drive)
    be = Backend(sm, **ss.BACKEND)
    be.set_save_dir(d)
    for lo, hi in ((0, 5), (5, SPLIT)):
        new_store(drive, lo, hi, sm)
        be.addKeyFrames()
        be.closeLoops()
    be.save()
    return dict(dir=d, be=be, sm=sm)


def test_session_a_wrote_the_raw_key_frames(drive, session_a):
    d = session_a["dir"]
    assert sorted(os.listdir(d)) == sorted([f"{i}.pcd" for i in range(SPLIT)] + ["tum.txt", "fg.g2o"])
    for i in range(SPLIT):
        assert ss.pcd_body(os.path.join(d, f"{i}.pcd")).tobytes() == drive["scans"][i].tobytes(), i      # raw: before the in-place filter
        assert session_a["sm"].keyFrame(i)[0].shape[0] < drive["scans"][i].shape[0]


def test_backend_load_equals_the_public_calls(drive, session_a):
    from simpleslam_amd import Backend, PoseGraph, ScanContext, SubMap
    from test_backend_gpu import contexts
    d = session_a["dir"]
    sm = SubMap()
    be = Backend(sm, **ss.BACKEND)
    stamps, info = be.load(d)
    # the same load, call by call
    want_stamps, poses = sr.load_tum(os.path.join(d, "tum.txt"))
    hand = SubMap()
    for i in range(SPLIT):
        hand.addKeyFrame(ss.pcd_body(os.path.join(d, f"{i}.pcd")), poses[i])
    sc = ScanContext()
    sc.addKeyFrames(hand, 0, SPLIT, grid_size=0.5)
    hand.downSampleKeyFrames(0, 0.5)
    g = PoseGraph()
    g.loadG2o(os.path.join(d, "fg.g2o"))
    assert stamps.tobytes() == want_stamps.tobytes() == np.arange(SPLIT, dtype=np.float64).tobytes()
    assert_same_store(sm, hand, "loaded store")
    assert contexts(be.sc).tobytes() == contexts(sc).tobytes() and len(be.sc) == SPLIT
    assert be.graph.size() == g.size() == session_a["be"].graph.size() == (SPLIT, 1, SPLIT - 1)
    assert be.graph.poses().tobytes() == g.poses().tobytes()
    assert info["keyframes"] == info["contexts"] == info["keyframes_added"] == SPLIT and set(info["load_seconds"]) == set(Backend.LOAD_STEPS)
    # the loaded session holds what session A held: the same filtered clouds and contexts, poses to the format's digits
    for i in range(SPLIT):
        assert sm.keyFrame(i)[0].tobytes() == session_a["sm"].keyFrame(i)[0].tobytes(), i
        assert np.abs(sm.keyFrame(i)[1][:3, 3] - session_a["sm"].keyFrame(i)[1][:3, 3]).max() <= 5e-4 + 1e-12
    assert contexts(be.sc).tobytes() == contexts(session_a["be"].sc).tobytes()
    # an event with nothing new changes nothing
    none = be.addKeyFrames()
    assert none["keyframes_added"] == 0 and none["keyframes"] == SPLIT and be.closeLoops()["candidates"] == 0


def test_a_second_session_closes_a_loop_onto_the_first(drive, session_a):
    """The test the feature exists for: the loop's old end is a key frame of session A, which ended with its process."""
    from simpleslam_amd import Backend, SubMap
    sm = SubMap()
    be = Backend(sm, **ss.BACKEND)
    be.load(session_a["dir"])
    new_store(drive, SPLIT, N, sm)
    add = be.addKeyFrames()
    assert add["keyframes_added"] == N - SPLIT and add["keyframes"] == add["contexts"] == N and add["factors_added"] == N - SPLIT
    before = sm.keyFrame(N - 1)[1]
    lc = be.closeLoops()
    loops = be.loops()
    for r in loops:
        print(f"loop cur {r['cur']} old {r['old']} converged {r['converged']} iterations {r['iterations']} fitness {r['fitness']:.4f} accepted {r['accepted']}")
    assert all(SPLIT <= r["cur"] < N for r in loops)      # only the new key frames are queries
    accepted = [r for r in loops if r["accepted"]]
    assert lc["accepted"] == len(accepted) >= 1
    assert any(r["old"] < SPLIT for r in accepted)
    assert be.graph.size() == (N, 1, N - 1 + len(accepted)) and len(be.sc) == N and sm.keyframes() == N
    after = sm.keyFrame(N - 1)[1]
    truth = drive["truth"][N - 1]
    e_before, e_after = float(np.linalg.norm(before[:3, 3] - truth[:3, 3])), float(np.linalg.norm(after[:3, 3] - truth[:3, 3]))
    print(f"newest key frame {e_before:.3f} m -> {e_after:.3f} m from its true pose")
    assert e_after < e_before


def test_without_a_save_directory_nothing_changes_and_no_file_appears(drive, session_a, tmp_path, monkeypatch):
    from simpleslam_amd import Backend
    from test_backend_gpu import Composed, contexts, store_poses
    monkeypatch.chdir(tmp_path)
    sm_a, sm_b = new_store(drive), new_store(drive)
    be = Backend(sm_a, **ss.BACKEND)
    ref = Composed(sm_b, detectors=0)
    be.set_save_dir("")
    for lo, hi in ((0, 5), (5, SPLIT)):
        new_store(drive, lo, hi, sm_a)
        new_store(drive, lo, hi, sm_b)
        info = be.addKeyFrames()
        delta = ref.add_keyframes()
        assert info["delta"].tobytes() == delta.tobytes()
        assert_same_store(sm_a, sm_b, f"{lo}:{hi}")
        assert contexts(be.sc).tobytes() == contexts(ref.sc).tobytes() and be.graph.poses().tobytes() == ref.g.poses().tobytes()
    assert os.listdir(tmp_path) == []
    # ... and a save directory is a side effect alone: session A, which had one, holds the same bytes and poses
    assert_same_store(sm_a, session_a["sm"], "with and without a save directory")
    from simpleslam_amd import PcrError
    with pytest.raises(PcrError, match="no save directory"):
        be.save()


def test_backend_load_refusals_change_nothing_and_a_good_load_follows(session_a, tmp_path):
    from simpleslam_amd import Backend, PcrError, PoseGraph, SubMap
    sm = SubMap()
    be = Backend(sm, **ss.BACKEND)
    seven = tmp_path / "seven"
    shutil.copytree(session_a["dir"], seven)
    g = PoseGraph()
    g.addPrior(np.eye(4), id=0)
    g.addPoses(np.array([ss.planar(float(i), 0, 0, 0) for i in range(SPLIT - 1)]))
    for i in range(1, SPLIT - 1):
        g.addOdomFactor(i - 1, i)
    g.saveG2o(str(seven / "fg.g2o"))
    with pytest.raises(PcrError, match="7 vertices.*8 key frames"):
        be.load(str(seven))
    assert sm.keyframes() == 0 and be.graph.size() == (0, 0, 0) and len(be.sc) == 0
    os.remove(seven / "fg.g2o")
    with pytest.raises(PcrError, match="fg.g2o.*pcr_map_load"):
        be.load(str(seven))
    assert sm.keyframes() == 0 and be.graph.size() == (0, 0, 0) and len(be.sc) == 0
    _stamps, info = be.load(session_a["dir"])
    assert info["keyframes"] == SPLIT and sm.keyframes() == SPLIT and be.graph.size() == (SPLIT, 1, SPLIT - 1)
    with pytest.raises(PcrError, match="freshly created or reset"):      # a second load needs a reset and an empty store
        be.load(session_a["dir"])
    assert sm.keyframes() == SPLIT
    be.reset()
    sm.clear()
    assert be.load(session_a["dir"])[1]["keyframes"] == SPLIT


def test_seq_harness_save_then_load_and_the_mirrors_check_program(gpu, tmp_path):
    """lib/seq_harness --save then --load (backend::Backend::setSaveDir / save / load of the C++ mirror) print the same key-frame count;
    lib/session_check map drives PCR::SubMap::save / load."""
    from simpleslam_amd import sequence
    exe = os.path.join(ROOT, "simpleslam_amd", "lib", "seq_harness")
    chk = os.path.join(ROOT, "simpleslam_amd", "lib", "session_check")
    assert os.path.exists(exe) and os.path.exists(chk), "seq_harness / session_check not built (run __graft_entry__.build())"
    scans, truth, cmds = sequence.make_drive(8, 20261005, map_points=120_000, beams=32, azimuths=512)
    names = []
    for k, s in enumerate(scans):
        np.ascontiguousarray(s, np.float32).tofile(tmp_path / f"scan{k:02d}.f32")
        names.append(str(tmp_path / f"scan{k:02d}.f32"))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "cmds.txt").write_text("".join(" ".join(repr(float(v)) for v in np.asarray(c).reshape(-1)) + "\n" for c in cmds))
    (tmp_path / "start.txt").write_text(" ".join(repr(float(v)) for v in np.asarray(truth[0]).reshape(-1)) + "\n")
    args = [exe, "loam"] + [str(tmp_path / n) for n in ("list.txt", "cmds.txt", "start.txt")]
    (tmp_path / "session").mkdir()
    out = subprocess.run(args + ["--save", str(tmp_path / "session")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    saved = [int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("saved keyframes ")]
    assert len(saved) == 1 and saved[0] >= 2
    assert sorted(os.listdir(tmp_path / "session")) == sorted([f"{i}.pcd" for i in range(saved[0])] + ["tum.txt", "fg.g2o"])
    out = subprocess.run(args + ["--load", str(tmp_path / "session")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    loaded = [int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("loaded keyframes ")]
    assert loaded == saved
    (tmp_path / "check").mkdir()
    out = subprocess.run([chk, "map", str(tmp_path / "check")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "session_check ok", out.stderr
