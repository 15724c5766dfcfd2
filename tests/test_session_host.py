"""The session's file formats in the library, on the CPU: pcr_tum_format byte for byte and pcr_tum_parse bit for bit against the numpy
restatement (session_ref.py), pcr_pcd_write / pcr_pcd_read over sizes, strides and non-finite rows, the writer against the C++ mirror's
pcp::savePCDFile, and the golden session tests/golden/session_small."""
import os
import subprocess

import numpy as np
import pytest

import session_ref as sr
import session_scene as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "simpleslam_amd", "lib", "session_check")


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", sorted(sr.POSES))
def test_tum_format_byte_for_byte_and_tum_parse_bit_for_bit(name, precise):
    from simpleslam_amd import tum_format, tum_parse
    stamp, T = sr.POSES[name]
    want = sr.tum_format(stamp, T, precise=precise)
    got = tum_format(stamp, T, precise=precise)
    assert got == want.encode()
    got_stamp, got_T = tum_parse(got)
    want_stamp, want_T = sr.tum_parse(want)
    assert got_stamp == want_stamp
    assert got_T.tobytes() == want_T.tobytes()      # (bits: a negative zero stays one)


def test_tum_parse_on_hand_written_lines():
    from simpleslam_amd import PcrError, tum_parse
    for line in ("1.5 1 2 3 0 0 0 1\n", "0 0 0 0 0 0 1 1", "  7.000 -0.000 0.000 -0.000 0.1 -0.2 0.3 0.9  \r\n", "1 2 3 4 0 0 0 1 trailing words",
                 "1e3 -2.5e-1 +3 4. .5 0 0 1"):
        got, want = tum_parse(line), sr.tum_parse(line)
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes(), line
    for line in ("", "\n", "   \t\r\n"):
        assert tum_parse(line) is None and sr.tum_parse(line) is None
    with pytest.raises(PcrError, match="holds 7.*1 2 3 4 0 0 0"):
        tum_parse("1 2 3 4 0 0 0\n")
    with pytest.raises(PcrError, match="holds 2"):
        tum_parse("1 2 three 4 0 0 0 1")


def test_tum_format_refusals():
    from simpleslam_amd import PcrError, tum_format
    stamp, T = sr.POSES["trace"]
    line = sr.tum_format(stamp, T).encode()
    assert tum_format(stamp, T, capacity=len(line) + 1) == line      # the line and its NUL fit exactly
    with pytest.raises(PcrError, match=f"takes {len(line) + 1} bytes"):
        tum_format(stamp, T, capacity=len(line))                     # one byte short
    for bad in (np.nan, np.inf):
        B = T.copy()
        B[1, 3] = bad
        with pytest.raises(PcrError, match="not finite"):
            tum_format(stamp, B)
        B = T.copy()
        B[2, 0] = bad
        with pytest.raises(PcrError, match="not finite"):
            tum_format(stamp, B, precise=True)
    with pytest.raises(PcrError, match="not finite"):
        tum_format(np.nan, T)


def _cloud(n, columns, seed=0):
    return ss.cloud(n, 40 + seed, stride_floats=columns)


@pytest.mark.parametrize("columns", [4, 8])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_pcd_round_trip_returns_the_bytes(tmp_path, n, columns):
    from simpleslam_amd import pcd_read, pcd_write
    a = _cloud(n, columns, n)
    if n >= 4:      # rows with NaN and inf travel as bytes: x, y, z or the intensity, either sign
        ii = 3 if columns == 4 else 4
        a[0, 0], a[1, 1], a[2, 2], a[3, ii] = np.nan, np.inf, -np.inf, np.nan
        a[4, :3] = np.nan
    path = str(tmp_path / "c.pcd")
    pcd_write(path, a)
    back = pcd_read(path, columns)
    assert back.shape == a.shape and back.tobytes() == a.tobytes()
    assert ss.pcd_body(path).tobytes() == np.ascontiguousarray(a[:, [0, 1, 2, 3 if columns == 4 else 4]]).tobytes()
    if n == 0:
        assert b"POINTS 0\n" in open(path, "rb").read()
    if n:      # the other layout reads the same file: the intensity moves, float 3 of a PointXYZI record is 1
        other = pcd_read(path, 12 - columns)
        assert other[:, :3].tobytes() == a[:, :3].tobytes()


def test_pcd_twelve_byte_points_have_no_intensity(tmp_path):
    from simpleslam_amd import pcd_read, pcd_write
    a = _cloud(9, 4)[:, :3].copy()
    pcd_write(str(tmp_path / "c.pcd"), a)
    assert (pcd_read(str(tmp_path / "c.pcd"), 4)[:, 3] == 0).all()
    assert pcd_read(str(tmp_path / "c.pcd"), 3).tobytes() == a.tobytes()


def test_pcd_read_refusals(tmp_path):
    import ctypes as C
    from simpleslam_amd import PcrError, load_library, pcd_read, pcd_write
    with pytest.raises(PcrError, match="cannot open .*nowhere.pcd"):
        pcd_read(str(tmp_path / "nowhere.pcd"))
    path = str(tmp_path / "c.pcd")
    pcd_write(path, _cloud(10, 4))
    L = load_library()
    out = np.full((9, 4), 7.0, np.float32)
    n = C.c_size_t(0)
    assert L.pcr_pcd_read(path.encode(), out.ctypes.data_as(C.c_void_p), 9, 16, C.byref(n)) != 0      # a capacity one point short
    assert n.value == 10 and (out == 7.0).all() and b"holds 10 points" in L.pcr_session_last_error()
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-5])
    with pytest.raises(PcrError, match="fewer than 10 binary records"):
        pcd_read(path)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_pcd_write_equals_the_mirrors_savePCDFile(tmp_path, n):
    from simpleslam_amd import pcd_write
    assert os.path.exists(CHECK), "session_check not built (run __graft_entry__.build())"
    a = _cloud(n, 4, n)
    if n > 2:
        a[1, 2], a[2, 3] = np.nan, np.inf
    a.tofile(tmp_path / "in.f32")
    r = subprocess.run([CHECK, "pcd", str(tmp_path / "in.f32"), str(tmp_path / "mirror.pcd")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    pcd_write(str(tmp_path / "lib.pcd"), a)
    assert open(tmp_path / "lib.pcd", "rb").read() == open(tmp_path / "mirror.pcd", "rb").read()


def test_the_golden_session_parses_to_its_arrays():
    from simpleslam_amd import PoseGraph, pcd_read, tum_parse
    want = np.load(os.path.join(ss.GOLDEN, "session_small.npz"))
    lines = open(os.path.join(ss.GOLDEN, "tum.txt")).read().splitlines()
    assert len(lines) == 3
    for i, line in enumerate(lines):
        stamp, T = tum_parse(line)
        assert stamp == want["stamps"][i] and T.tobytes() == want["poses"][i].tobytes()
        c = pcd_read(os.path.join(ss.GOLDEN, f"{i}.pcd"))
        assert c.shape[0] <= 64 and c.tobytes() == want[f"cloud{i}"].tobytes()
    g = PoseGraph(device=-2)      # a host graph: no device
    g.loadG2o(os.path.join(ss.GOLDEN, "fg.g2o"))
    assert g.size() == tuple(want["graph_size"]) == (3, 1, 2)
    assert g.poses().tobytes() == want["graph_poses"].tobytes()
    # ... and the scene it was written from gives the same files again
    clouds, poses, stamps = ss.small_session()
    for i in range(3):
        assert clouds[i].tobytes() == want[f"cloud{i}"].tobytes()
    assert "".join(sr.tum_format(s, T) for s, T in zip(stamps, poses)) == open(os.path.join(ss.GOLDEN, "tum.txt")).read()
    assert sum(os.path.getsize(os.path.join(ss.GOLDEN, f)) for f in os.listdir(ss.GOLDEN)) < 16 * 1024
