"""A session's text formats restated in numpy and Python floats: utils::file::writeAsTum and loadFromTum (common/utils/File.hpp:49-95),
Eigen::Quaternion(R) and Eigen's toRotationMatrix.  Nothing of oracle/ and nothing of the library: the CPU suite checks this file on
hand-worked lines (test_session_ref.py) and the library against this file (test_session_host.py, test_session_gpu.py).

Poses are 4x4 numpy arrays, row by row as numpy holds them.  Every operation is one IEEE double operation in the order written: the C code
(compiled without contraction) and this file give the same bits."""
import math

import numpy as np

POSES = {}      # name -> (stamp, 4x4): the poses the tests share, filled below


def quaternion_of(R):
    """Eigen::Quaternion(R) (Quaternion.h: quaternionbase_assign_impl<Other, 3, 3>), NOT normalised -> (x, y, z, w)"""
    m = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    q = [0.0, 0.0, 0.0, 0.0]
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return tuple(q)


def branch_of(R):
    """which branch quaternion_of takes: 'trace', or the index of the largest diagonal entry"""
    if float(R[0, 0]) + float(R[1, 1]) + float(R[2, 2]) > 0:
        return "trace"
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i


def rotation_of(x, y, z, w):
    """Eigen's QuaternionBase::toRotationMatrix of the quaternion as it stands (no normalisation)"""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype=np.float64)


def tum_format(stamp, T, precise=False):
    """one line of writeAsTum: fmt's {:.3f} / {:.6f} round as printf's %.3f / %.6f do (correctly, from the exact binary value)"""
    x, y, z, w = quaternion_of(T[:3, :3])
    v = (float(stamp), float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), x, y, z, w)
    if precise:
        return " ".join("%.17g" % a for a in v) + "\n"
    return "%.3f %.3f %.3f %.3f %.6f %.6f %.6f %.6f\n" % v


def tum_parse(line):
    """loadFromTum's body for one line -> (stamp, 4x4), None for a blank line; ValueError (with the line) for fewer than eight numbers.
    pose = identity . translate(t) . rotate(q): the translation is t, the rotation toRotationMatrix(q) of q as read."""
    tok = line.split()
    if not tok:
        return None
    v = []
    for t in tok[:8]:
        try:
            v.append(float(t))
        except ValueError:
            break
    if len(v) < 8:
        raise ValueError(f"a tum line holds 8 numbers, this one {len(v)}: {line!r}")
    T = np.eye(4)
    T[:3, :3] = rotation_of(*v[4:8])
    T[:3, 3] = v[1:4]
    return v[0], T


def load_tum(path):
    """every non-blank line of a tum.txt -> (stamps (n,), poses (n, 4, 4))"""
    stamps, poses = [], []
    with open(path) as f:
        for line in f:
            r = tum_parse(line)
            if r is not None:
                stamps.append(r[0])
                poses.append(r[1])
    return np.array(stamps, dtype=np.float64), np.array(poses, dtype=np.float64).reshape(-1, 4, 4)


def _rot(axis, deg):
    """Rodrigues' rotation about a unit axis"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = math.radians(deg)
    return np.eye(3) + math.sin(r) * K + (1 - math.cos(r)) * (K @ K)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


# trace > 0; one pose per largest-diagonal branch (rotations by 170 degrees about an axis near x, y, z: the trace is 1 + 2 cos < 0 and the
# largest diagonal entry is the axis's); a half turn; a stamp of 0; a negative zero translation
POSES["trace"] = (1234.5678, _pose(_rot([0.2, -0.3, 1.0], 35.0), [12.3456789, -0.000449, 1000.0005]))
POSES["diag_x"] = (1.0, _pose(_rot([1.0, 0.1, -0.05], 170.0), [-3.25, 4.125, 0.0625]))
POSES["diag_y"] = (2.5, _pose(_rot([0.1, 1.0, 0.08], 170.0), [100.0004, -100.0006, 7.0]))
POSES["diag_z"] = (3.75, _pose(_rot([-0.07, 0.1, 1.0], 170.0), [0.0015, 0.0025, -0.0035]))
POSES["half_turn"] = (4.0, _pose(np.diag([-1.0, -1.0, 1.0]), [1.0, 2.0, 3.0]))
POSES["stamp_zero"] = (0.0, _pose(np.eye(3), [0.5, 0.25, 0.125]))
POSES["negative_zero"] = (7.0, _pose(_rot([0.0, 0.0, 1.0], 90.0), [-0.0, 0.0, -0.0004]))
