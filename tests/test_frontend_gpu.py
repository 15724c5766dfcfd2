"""The per-scan loop in the library (pcr_frontend_*, simpleslam_amd.pcr.Frontend, PCR::Frontend, lib/seq_harness) against the Python loop the other
tests trust (simpleslam_amd.sequence.drive over GpuFront): the same drive as tests/test_sequence_gpu.py, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "seq_harness")


@pytest.fixture(scope="module")
def drive_inputs(gpu):
    import torch
    from simpleslam_amd import sequence
    scans, truth, cmds = sequence.make_drive(14, 20261005, map_points=120_000, beams=32, azimuths=512)
    return dict(scans=scans, truth=truth, cmds=cmds, d_scans=[torch.from_numpy(s).cuda() for s in scans])


@pytest.fixture(scope="module")
def python_drive(drive_inputs):
    """drive() over GpuFront, computed once per (method, mobile) and shared."""
    from simpleslam_amd import make_register, sequence
    done = {}

    def get(method, mobile=False):
        if (method, mobile) not in done:
            d = drive_inputs
            done[(method, mobile)] = sequence.drive(sequence.GpuFront(make_register(method)), d["d_scans"], d["cmds"], d["truth"][0], mobile=mobile)
        return done[(method, mobile)]
    return get


def assert_same_drive(a, b):
    assert len(a["poses"]) == len(b["poses"])
    for k, (p, q) in enumerate(zip(a["poses"], b["poses"])):
        np.testing.assert_array_equal(p, q, err_msg=f"pose of scan {k}")
    for key in ("converged", "iterations", "keyframes", "updates", "submap_points"):
        assert a[key] == b[key], key


@pytest.mark.parametrize("method", ["loam", "ndt", "vgicp", "gicp", "liorf"])
def test_the_library_loop_equals_the_python_loop(drive_inputs, python_drive, method):
    from simpleslam_amd import Frontend, make_register, sequence
    d = drive_inputs
    got = sequence.drive_frontend(Frontend(make_register(method)), d["d_scans"], d["cmds"], d["truth"][0])
    ref = python_drive(method)
    assert_same_drive(got, ref)
    assert ref["keyframes"] >= 2 and ref["updates"] >= 2 and any(ref["iterations"])      # (the drive exercises what it compares)


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_mobile_projection_inside_the_loop(drive_inputs, python_drive, method):
    from simpleslam_amd import Frontend, make_register, sequence
    d = drive_inputs
    got = sequence.drive_frontend(Frontend(make_register(method), mobile=True), d["d_scans"], d["cmds"], d["truth"][0])
    assert_same_drive(got, python_drive(method, mobile=True))
    for k, T in enumerate(got["poses"]):
        assert T[2, 3] == 0.0, k
        assert T[0, 2] == 0.0 and T[1, 2] == 0.0 and T[2, 0] == 0.0 and T[2, 1] == 0.0, k
        assert abs(T[2, 2] - 1.0) <= 2.3e-16, k
    # the world's trajectory has a non-zero z: the flag does something
    plain = python_drive(method)
    assert not all(np.array_equal(a, b) for a, b in zip(got["poses"], plain["poses"]))


def test_reset_and_prefetch_change_nothing(drive_inputs, python_drive):
    from simpleslam_amd import Frontend, make_register, sequence
    d = drive_inputs
    fe = Frontend(make_register("loam"))
    first = sequence.drive_frontend(fe, d["d_scans"], d["cmds"], d["truth"][0])
    fe.reset()
    again = sequence.drive_frontend(fe, d["d_scans"], d["cmds"], d["truth"][0])
    fe.reset()
    ahead = sequence.drive_frontend(fe, d["d_scans"], d["cmds"], d["truth"][0], prefetch=True)
    assert_same_drive(again, first)
    assert_same_drive(ahead, first)
    assert_same_drive(first, python_drive("loam"))


def _product(a, b):
    """rows times columns in plain Python floats, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3: seq_harness's product."""
    return [[((a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c]) + a[r][3] * b[3][c] for c in range(4)] for r in range(4)]


def _write_inputs(d, tmp_path):
    names = []
    for k, s in enumerate(d["scans"]):
        f = tmp_path / f"scan{k:02d}.f32"
        np.ascontiguousarray(s, np.float32).tofile(f)
        names.append(str(f))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "cmds.txt").write_text("".join(" ".join(repr(float(v)) for v in np.asarray(c).reshape(-1)) + "\n" for c in d["cmds"]))
    (tmp_path / "start.txt").write_text(" ".join(repr(float(v)) for v in np.asarray(d["truth"][0]).reshape(-1)) + "\n")
    return [str(tmp_path / n) for n in ("list.txt", "cmds.txt", "start.txt")]


def _xyzi32(scan):
    """The scan as the harness holds it: pcl::PointXYZI records, x y z 1 | intensity 0 0 0."""
    out = np.zeros((scan.shape[0], 8), np.float32)
    out[:, :3] = scan[:, :3]
    out[:, 3] = 1.0
    out[:, 4] = scan[:, 3]
    return out


@pytest.mark.parametrize("mobile", [False, True])
def test_seq_harness_equals_the_python_binding(drive_inputs, tmp_path, mobile):
    """lib/seq_harness is built over PCR::Frontend (the C++ mirror), so this covers the mirror too."""
    import torch
    from simpleslam_amd import Frontend, make_register
    assert os.path.exists(EXE), "seq_harness not built (run __graft_entry__.build())"
    d = drive_inputs
    args = _write_inputs(d, tmp_path)
    out = subprocess.run([EXE, "loam"] + args + (["--mobile"] if mobile else []), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("scan ")]
    assert len(rows) == len(d["scans"]) and [int(r[1]) for r in rows] == list(range(len(rows)))
    assert any(ln.startswith("summary first scans %d " % len(rows)) for ln in out.stdout.splitlines())

    fe = Frontend(make_register("loam"), mobile=mobile)
    pose = [[float(v) for v in row] for row in np.asarray(d["truth"][0])]
    for k, s in enumerate(d["scans"]):
        init = _product(pose, [[float(v) for v in row] for row in np.asarray(d["cmds"][k])])
        T, info = fe.step(torch.from_numpy(_xyzi32(s)).cuda(), np.array(init))
        got = np.array([float.fromhex(v) for v in rows[k][2:18]]).reshape(4, 4)
        np.testing.assert_array_equal(got, T, err_msg=f"pose of scan {k}")
        assert [int(v) for v in rows[k][18:23]] == [info["converged"], info["iterations"], info["keyframe_added"], info["update_queued"], info["n_submap"]], k
        pose = [[float(v) for v in row] for row in T]
    assert sum(int(r[20]) for r in rows) >= 2 and any(int(r[19]) for r in rows)


def test_seq_harness_refuses_bad_input(drive_inputs, tmp_path):
    d = drive_inputs
    args = _write_inputs(dict(d, scans=d["scans"][:2]), tmp_path)
    bad = subprocess.run([EXE, "loam", args[0]], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stderr
    bad = subprocess.run([EXE, "loam"] + args + ["--reps"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stderr
    bad = subprocess.run([EXE, "loam"] + args + ["--grid", "-1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--grid" in bad.stderr
    bad = subprocess.run([EXE, "icp"] + args, capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "is not exist" in bad.stderr
    (tmp_path / "missing.txt").write_text(str(tmp_path / "scan00.f32") + "\n" + str(tmp_path / "nowhere.f32") + "\n")
    bad = subprocess.run([EXE, "loam", str(tmp_path / "missing.txt")] + args[1:], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "nowhere.f32" in bad.stderr


def test_refused_scans_and_a_step_after_a_failed_step(drive_inputs):
    import torch
    from simpleslam_amd import Frontend, SubMap, make_register
    from simpleslam_amd.pcr import PcrError
    d = drive_inputs
    fe = Frontend(make_register("loam"))
    with pytest.raises(PcrError, match="0 points"):
        fe.step(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), np.eye(4))
    with pytest.raises(PcrError, match="0 points"):
        fe.prefetch(torch.zeros((0, 4), dtype=torch.float32, device="cuda"))
    # a refused argument leaves the loop as it was: the drive starts normally
    T, info = fe.step(d["d_scans"][0], d["truth"][0])
    np.testing.assert_array_equal(T, d["truth"][0])
    assert (info["registered"], info["converged"], info["iterations"], info["keyframe_added"], info["update_queued"], info["n_submap"]) == (0, 1, 0, 1, 1, 0)
    assert fe.finish() > 0
    # a scan in another point layout than the map's key frames
    with pytest.raises(PcrError, match="point layout"):
        fe.step(torch.from_numpy(_xyzi32(d["scans"][1])).cuda(), d["truth"][1])

    # an inner call that fails -- a view cannot take key frames -- is reported under the step's name; the next step reports that failure, no crash
    parent = SubMap()
    broken = Frontend(make_register("loam"), submap=parent.view())
    with pytest.raises(PcrError, match="^add_keyframe: .*view"):
        broken.step(d["d_scans"][0], d["truth"][0])
    with pytest.raises(PcrError, match="earlier step.*add_keyframe"):
        broken.step(d["d_scans"][1], d["truth"][1])
    with pytest.raises(PcrError, match="earlier step.*add_keyframe"):
        broken.prefetch(d["d_scans"][1])
