"""pcr_frontend_closest: the key frame nearest to each key frame the front end adds (mClosestKfIdx), recomputed here from the key-frame
poses, and a recording that changes nothing of the drive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drive_inputs(gpu):
    import torch
    from simpleslam_amd import sequence
    scans, truth, cmds = sequence.make_drive(14, 20261005, map_points=120_000, beams=32, azimuths=512)
    return dict(truth=truth, cmds=cmds, d_scans=[torch.from_numpy(s).cuda() for s in scans])


def drive_step_by_step(fe, d, ask):
    """drive_frontend's loop, with closest() read after every step when `ask` -> (poses, infos, closest per step, key-frame poses as added)"""
    pose = np.array(d["truth"][0], float)
    poses, infos, seen, kf_poses = [], [], [], []
    for k, scan in enumerate(d["d_scans"]):
        pose, info = fe.step(scan, pose @ d["cmds"][k])
        poses.append(pose)
        infos.append({f: v for f, v in info.items() if f != "seconds"})
        if info["keyframe_added"]:
            kf_poses.append(pose.copy())
        if ask:
            seen.append(fe.closest())
    fe.finish()
    return poses, infos, seen, kf_poses


def test_closest_is_the_argmin_and_recording_changes_nothing(drive_inputs):
    from simpleslam_amd import Frontend, make_register
    d = drive_inputs
    fe = Frontend(make_register("loam"))
    assert fe.closest().size == 0
    poses, infos, seen, kf_poses = drive_step_by_step(fe, d, ask=True)
    quiet = Frontend(make_register("loam"))
    q_poses, q_infos, _, _ = drive_step_by_step(quiet, d, ask=False)
    for k, (a, b) in enumerate(zip(poses, q_poses)):
        np.testing.assert_array_equal(a, b, err_msg=f"pose of scan {k}")
    assert infos == q_infos

    got = fe.closest()
    assert len(kf_poses) >= 3 and got.size == len(kf_poses) == infos[-1]["keyframes"]
    pos = np.array([P[:3, 3] for P in kf_poses])
    want = [-1]
    for i in range(1, len(pos)):
        dlt = pos[:i] - pos[i]
        d2 = (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]
        want.append(int(np.argmin(d2)))      # (the first of equal minima: the lowest index)
    assert got.tolist() == want
    # the list grows by one entry per key frame and never rewrites one
    n = 0
    for info, c in zip(infos, seen):
        n += info["keyframe_added"]
        assert c.tolist() == want[:n]
    np.testing.assert_array_equal(quiet.closest(), got)
    fe.reset()
    assert fe.closest().size == 0
