"""tests/session_ref.py -- the numpy restatement of writeAsTum, loadFromTum, Eigen::Quaternion(R) and toRotationMatrix -- on lines worked
out by hand, on both kinds of branch of the quaternion's construction, and on the bounds the format itself sets on parse(format(pose))."""
import math

import numpy as np
import pytest

import session_ref as sr


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def test_hand_worked_lines_of_writeAsTum():
    # identity: trace 3 > 0, t = sqrt(4) = 2, w = 1, x = y = z = 0 * 0.25
    assert sr.tum_format(0.0, pose(np.eye(3), [0.5, 0.25, 0.125])) == "0.000 0.500 0.250 0.125 0.000000 0.000000 0.000000 1.000000\n"
    # a half turn about z, diag(-1, -1, 1): trace -1, largest diagonal entry 2, t = sqrt(1 + 1 + 1 + 1) = 2, z = 1, w = (R10 - R01) / 4 = 0
    assert sr.tum_format(4.0, pose(np.diag([-1.0, -1.0, 1.0]), [1, 2, 3])) == "4.000 1.000 2.000 3.000 0.000000 0.000000 1.000000 0.000000\n"
    # ... about x, diag(1, -1, -1): largest diagonal entry 0, x = 1; ... about y
    assert sr.tum_format(1.0, pose(np.diag([1.0, -1.0, -1.0]), [0, 0, 0])) == "1.000 0.000 0.000 0.000 1.000000 0.000000 0.000000 0.000000\n"
    assert sr.tum_format(1.0, pose(np.diag([-1.0, 1.0, -1.0]), [0, 0, 0])) == "1.000 0.000 0.000 0.000 0.000000 1.000000 0.000000 0.000000\n"
    # a quarter turn about z, [[0, -1, 0], [1, 0, 0], [0, 0, 1]]: trace 1, t = sqrt(2), w = sqrt(2) / 2, z = (1 + 1) / (2 sqrt(2)); a negative zero
    # and a translation that rounds to it keep their sign, as fmt and printf both write them
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert sr.tum_format(7.0, pose(Rz, [-0.0, 0.0, -0.0004])) == "7.000 -0.000 0.000 -0.000 0.000000 0.000000 0.707107 0.707107\n"
    # rounding acts on the EXACT binary value: the doubles nearest 0.0005, 0.0015 and 0.0025 all lie a little above the tie, so all round up
    # (5.00000000000000010e-4, 1.50000000000000003e-3, 2.50000000000000005e-3); 0.125 is exact and %.2f would tie, %.3f writes it whole
    assert sr.tum_format(0.0, pose(np.eye(3), [0.0005, 0.0015, 0.0025])).split()[1:4] == ["0.001", "0.002", "0.003"]


def test_hand_worked_lines_of_loadFromTum():
    stamp, T = sr.tum_parse("1.5 1 2 3 0 0 0 1\n")
    assert stamp == 1.5
    np.testing.assert_array_equal(T, pose(np.eye(3), [1, 2, 3]))
    _, T = sr.tum_parse("0 0 0 0 0 0 1 0")
    np.testing.assert_array_equal(T, pose(np.diag([-1.0, -1.0, 1.0]), [0, 0, 0]))
    # NOT normalised: q = (0, 0, 1, 1) has tz = twz = tzz = 2 -> R00 = R11 = 1 - 2, R01 = -2, R10 = 2 (a quarter turn scaled by 2 and sheared)
    _, T = sr.tum_parse("0 0 0 0 0 0 1 1")
    np.testing.assert_array_equal(T[:3, :3], [[-1.0, -2.0, 0.0], [2.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    # what follows the eighth number is ignored; a blank line is skipped; seven numbers are an error that shows the line
    assert sr.tum_parse("1 2 3 4 0 0 0 1 trailing words")[0] == 1.0
    assert sr.tum_parse("") is None and sr.tum_parse("   \t\r\n") is None
    with pytest.raises(ValueError, match="1 2 3 4 0 0 0"):
        sr.tum_parse("1 2 3 4 0 0 0\n")
    # a negative zero translation is read as one
    _, T = sr.tum_parse("7.000 -0.000 0.000 -0.000 0 0 0 1")
    assert math.copysign(1.0, T[0, 3]) == -1.0 and math.copysign(1.0, T[1, 3]) == 1.0 and math.copysign(1.0, T[2, 3]) == -1.0


def test_the_shared_poses_cover_every_branch():
    assert sr.branch_of(sr.POSES["trace"][1]) == "trace"
    assert [sr.branch_of(sr.POSES[k][1]) for k in ("diag_x", "diag_y", "diag_z", "half_turn")] == [0, 1, 2, 2]
    assert sr.POSES["stamp_zero"][0] == 0.0
    T = sr.POSES["negative_zero"][1]
    assert T[0, 3] == 0.0 and math.copysign(1.0, T[0, 3]) == -1.0
    for name, (_stamp, T) in sr.POSES.items():      # proper rotations: the quaternion has unit norm to rounding
        assert abs(np.linalg.norm(sr.quaternion_of(T[:3, :3])) - 1.0) < 1e-14, name
        np.testing.assert_allclose(sr.rotation_of(*sr.quaternion_of(T[:3, :3])), T[:3, :3], atol=1e-14, err_msg=name)


@pytest.mark.parametrize("name", sorted(sr.POSES))
def test_parse_of_format_stays_within_the_digits_written(name):
    """%.3f keeps a number within half a unit of its third decimal, 5e-4; %.6f within 5e-7.  These follow from the digits, not from a run.
    (The decimal-to-binary step of the reader adds half an ulp of a number below 1 100, 1.2e-13, which the comparison allows for.)"""
    stamp, T = sr.POSES[name]
    line = sr.tum_format(stamp, T)
    got_stamp, got = sr.tum_parse(line)
    assert abs(got_stamp - stamp) <= 5e-4 + 1.2e-13
    assert np.abs(got[:3, 3] - T[:3, 3]).max() <= 5e-4 + 1.2e-13
    q_written = np.array([float(t) for t in line.split()[4:8]])
    assert np.abs(q_written - np.array(sr.quaternion_of(T[:3, :3]))).max() <= 5e-7 + 1.2e-13
    # precise: 17 significant digits identify a double, so the stamp, the translation and the quaternion come back bit for bit
    line = sr.tum_format(stamp, T, precise=True)
    got_stamp, got = sr.tum_parse(line)
    assert got_stamp == stamp
    assert got[:3, 3].tobytes() == T[:3, 3].tobytes()
    assert np.array([float(t) for t in line.split()[4:8]]).tobytes() == np.array(sr.quaternion_of(T[:3, :3])).tobytes()
    np.testing.assert_array_equal(got[:3, :3], sr.rotation_of(*sr.quaternion_of(T[:3, :3])))
