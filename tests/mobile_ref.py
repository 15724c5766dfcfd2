"""trans::SixDof2Mobile (reference common/geometry/trans.hpp:68-86), restated step by step in Eigen's order of operations: the reference for
pcr_pose_to_mobile.  Scalars in Python floats (IEEE double, no contraction); sqrt, atan2, sin and cos are the C library's (math)."""
import math

import numpy as np


def quaternion(m):
    """Eigen's Quaternion(Matrix3) -> (branch, w, [x, y, z]).  branch: 'trace', or 'diag0' / 'diag1' / 'diag2' by the diagonal element chosen."""
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
        return "trace", w, q
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    w = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return "diag%d" % i, w, q


def angle_axis(w, q):
    """Eigen's AngleAxis(Quaternion) -> (angle, axis, zero: the vector part had norm 0, w_negative)."""
    n = math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    if n != 0.0:
        angle = 2.0 * math.atan2(n, abs(w))
        if w < 0.0:
            n = -n
        return angle, [q[0] / n, q[1] / n, q[2] / n], False, w < 0.0
    return 0.0, [1.0, 0.0, 0.0], True, False


def six_dof_to_mobile(T):
    """-> (4x4 result, dict(quat = the quaternion's branch, zero_axis, w_negative, about_z = the rotation was kept, axis_z, angle))."""
    T = np.asarray(T, np.float64)
    m = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    branch, w, q = quaternion(m)
    angle, axis, zero, wneg = angle_axis(w, q)
    out = np.eye(4)
    out[0, 3] = T[0, 3]
    out[1, 3] = T[1, 3]
    tmp = axis[2]
    about_z = abs(tmp) > 0.95
    if about_z:
        a = math.copysign(1.0, tmp)
        c, s = math.cos(angle), math.sin(angle)
        out[0, 0] = out[1, 1] = c
        out[0, 1] = -(a * s)
        out[1, 0] = a * s
        out[2, 2] = (1.0 - c) + c
    return out, dict(quat=branch, zero_axis=zero, w_negative=wneg, about_z=about_z, axis_z=tmp, angle=angle)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def random_rotation(rng):
    """A uniformly distributed rotation from a normalised Gaussian quaternion."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose(R, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T
