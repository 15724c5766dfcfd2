"""Scenes of the session tests (test_session_host.py, test_session_gpu.py): the small store whose key-frame sizes sit at the copy's and the
filter's edges, the 12-key-frame drive out and back along a street that a second session closes a loop on, and the golden session
tests/golden/session_small (written by write_small_session below, on the CPU, from a seeded scene)."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "session_small")
STORE_SIZES = (0, 1, 63, 64, 300)      # empty frame, single point, one short of a wave, a wave, more than one block of the filter's kernels
N_KF, SPLIT = 12, 8                    # the drive's key frames; session A takes [0, SPLIT)


def cloud(n, seed, stride_floats=4):
    """n seeded points in a 20 m x 20 m x 3 m box, x y z intensity (4 floats) or pcl::PointXYZI records (8 floats: x y z 1 intensity 0 0 0)"""
    rng = np.random.default_rng(seed)
    xyzi = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(0, 3, (n, 1)), rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)
    if stride_floats == 4:
        return np.ascontiguousarray(xyzi)
    out = np.zeros((n, stride_floats), np.float32)
    out[:, :3], out[:, 3], out[:, 4] = xyzi[:, :3], 1.0, xyzi[:, 3]
    return out


def planar(x, y, z, yaw_deg):
    a = math.radians(yaw_deg)
    T = np.eye(4)
    T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    T[:3, 3] = [x, y, z]
    return T


def store_scene():
    """the five key frames of the store tests -> (clouds, poses, stamps)"""
    clouds = [cloud(n, 100 + k) for k, n in enumerate(STORE_SIZES)]
    poses = [planar(1.5 * k, -0.75 * k, 0.125 * k, 25.0 * k - 40.0) for k in range(len(STORE_SIZES))]
    stamps = np.array([0.0, 0.1, 12.5, 1000.004, 1700000000.25])
    return clouds, poses, stamps


def pcd_body(path):
    """the records of a binary x y z intensity PCD as this project writes it, read without the library -> (n, 4) float32"""
    raw = open(path, "rb").read()
    mark = b"DATA binary\n"
    at = raw.index(mark) + len(mark)
    header = raw[:at].decode()
    n = int([ln.split()[1] for ln in header.splitlines() if ln.startswith("POINTS")][0])
    assert "FIELDS x y z intensity" in header and len(raw) - at == 16 * n, path
    return np.frombuffer(raw[at:], np.float32).reshape(n, 4).copy()


# ---- the drive: out along the street y = 100 and back again, so that the second half revisits the first ----
def course(k):
    """world (x, y, heading) of key frame k: 2 m apart from x = 104 to x = 116, a turn on the spot, and back along the same lane"""
    if k <= 6:
        return 104.0 + 2.0 * k, 100.0, 0.0
    return 104.0 + 2.0 * (12 - k), 100.0, 180.0


def drift(k):
    """what the odometry has accumulated by key frame k, applied on the map side: half a metre and a third of a degree by the end"""
    a = math.radians(0.03 * k)
    D = np.eye(4)
    D[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    D[:3, 3] = [0.04 * k, -0.025 * k, 0.0]
    return D


def build_drive(beams=8, azimuths=120):
    import global_reloc_scene as grs
    world, _ = grs.asymmetric_world(300_000, seed=3)
    truth = [grs.planar_pose(world, *course(k)) for k in range(N_KF)]
    scans = [np.ascontiguousarray(grs.scan_at(world, T, seed=900 + k, beams=beams, azimuths=azimuths)) for k, T in enumerate(truth)]
    assert max(len(s) for s in scans) <= beams * azimuths <= 2000
    poses = [drift(k) @ T for k, T in enumerate(truth)]
    return dict(truth=truth, scans=scans, poses=poses)


# the back end of the drive: the distance detector over so short a drive (ScanContext's query leaves out the 40 newest key frames)
BACKEND = dict(detectors=4, dist_radius=2.0, dist_exclude_recent=3)


# ---- the golden session ----
def small_session():
    """three key frames of 40, 64 and 7 points, their poses and stamps, and a graph over them: prior on 0, edges 0-1, 1-2"""
    clouds = [cloud(n, 7 + k) for k, n in enumerate((40, 64, 7))]
    poses = [planar(0.0, 0.0, 0.0, 0.0), planar(1.25, 0.5, 0.0, 10.0), planar(2.5, 1.5, 0.125, 200.0)]
    stamps = np.array([0.0, 0.5, 1.75])
    return clouds, poses, stamps


def write_small_session(directory=GOLDEN):
    """tests/golden/session_small by this project's own code, on the CPU (a host graph: no device).  Run once when the formats change:
    python -c "import sys; sys.path.insert(0, 'tests'); import session_scene; session_scene.write_small_session()" """
    import session_ref as sr
    from simpleslam_amd import PoseGraph, pcd_write, tum_format
    os.makedirs(directory, exist_ok=True)
    clouds, poses, stamps = small_session()
    for i, c in enumerate(clouds):
        pcd_write(os.path.join(directory, f"{i}.pcd"), c)
    with open(os.path.join(directory, "tum.txt"), "wb") as f:
        for s, T in zip(stamps, poses):
            f.write(tum_format(s, T))
    g = PoseGraph(device=-2)
    g.addPrior(poses[0], id=0)
    g.addPoses(np.array(poses))
    for i in (1, 2):
        g.addBetween(i - 1, i, np.linalg.inv(poses[i - 1]) @ poses[i])
    g.saveG2o(os.path.join(directory, "fg.g2o"))
    g = PoseGraph(device=-2)      # (what the file gives back: 17 digits of the quaternion, not the matrix that went in)
    g.loadG2o(os.path.join(directory, "fg.g2o"))
    got_stamps, got_poses = sr.load_tum(os.path.join(directory, "tum.txt"))
    np.savez(os.path.join(directory, "session_small.npz"), stamps=got_stamps, poses=got_poses, graph_poses=g.poses(), graph_size=np.array(g.size()),
             **{f"cloud{i}": c for i, c in enumerate(clouds)})
