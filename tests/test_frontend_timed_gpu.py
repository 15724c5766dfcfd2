"""pcr_frontend_step_timed against what it is defined as -- pcr_deskew into a device buffer, then pcr_frontend_step(on_device = 1) on that buffer --
over a six-scan drive with small scans: poses, the counts of pcr_frontend_info and the stored key frames, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
AZ = 256
INFO = ("registered", "converged", "iterations", "keyframe_added", "update_queued", "n_filtered", "n_submap", "keyframes", "updates")


@pytest.fixture(scope="module")
def drive_inputs(gpu):
    """Six scans of 4 096 points, 0.7 m apart (key frames at scans 0, 2 and 4 under the gap of 1 m), each with one time per azimuth column over a
    sweep of 0.1 s and a motion of three control poses that ends at the scan's own pose (t_ref at the end)."""
    import torch
    from simpleslam_amd import sequence, synth
    scans, truth, cmds = sequence.make_drive(6, 20261021, map_points=60_000, beams=16, azimuths=AZ, step=0.7)
    n = scans[0].shape[0]
    times = (0.1 * (np.arange(n) % AZ) / AZ).astype(np.float32)
    stamps = np.array([0.0, 0.04, 0.1])
    motions = []
    for k in range(len(scans)):
        xi = np.array([2.0, 0.1 * k, 0.0, 0.0, 0.01, 0.5 - 0.05 * k])
        motions.append(np.stack([synth.se3_exp(xi * (s - 0.1)) for s in stamps]))
    return dict(scans=scans, truth=truth, cmds=cmds, d_scans=[torch.from_numpy(s).cuda() for s in scans], times=times, d_times=torch.from_numpy(times).cuda(),
                stamps=stamps, motions=motions)


def _keyframes(submap):
    return [submap.keyFrame(i) for i in range(submap.keyframes())]


def _drive(step, d):
    pose = np.array(d["truth"][0], float)
    poses, infos = [], []
    for k in range(len(d["scans"])):
        pose, info = step(k, pose @ d["cmds"][k])
        poses.append(pose)
        infos.append(info)
    return poses, infos


@pytest.mark.parametrize("method", ["loam", "vgicp"])
def test_step_timed_is_deskew_then_step(drive_inputs, method):
    from simpleslam_amd import Frontend, deskew, make_register
    d = drive_inputs
    fe = Frontend(make_register(method))
    got_poses, got_infos = _drive(lambda k, init: fe.stepTimed(d["d_scans"][k], init, d["motions"][k], d["stamps"], times=d["d_times"], t_ref=0.1), d)
    fe.finish()

    ref = Frontend(make_register(method))

    def by_hand(k, init):
        out, dinfo = deskew(ref.reg, d["d_scans"][k], d["motions"][k], d["stamps"], times=d["d_times"], t_ref=0.1)
        pose, info = ref.step(out, init)
        info["deskew"] = dinfo
        return pose, info
    want_poses, want_infos = _drive(by_hand, d)
    ref.finish()

    for k, (p, q) in enumerate(zip(got_poses, want_poses)):
        np.testing.assert_array_equal(p, q, err_msg=f"pose of scan {k}")
    for k, (a, b) in enumerate(zip(got_infos, want_infos)):
        assert [a[f] for f in INFO] == [b[f] for f in INFO], k
        assert a["deskew"] == b["deskew"] == dict(before=0, after=0, nonfinite=0, ref_clamped=0), k
    kf_got, kf_want = _keyframes(fe.map), _keyframes(ref.map)
    assert len(kf_got) == len(kf_want) >= 2
    for i, ((c1, p1), (c2, p2)) in enumerate(zip(kf_got, kf_want)):
        np.testing.assert_array_equal(c1.view(np.uint32), c2.view(np.uint32), err_msg=f"key frame {i}")
        np.testing.assert_array_equal(p1, p2, err_msg=f"pose of key frame {i}")
    # the drive exercises what it compares: registrations ran, and the key frames are the DESKEWED scans, not the raw ones
    assert any(i["registered"] and i["iterations"] for i in got_infos)
    assert not np.array_equal(kf_got[0][0].view(np.uint32), d["scans"][0].view(np.uint32))


def test_an_identity_motion_is_the_plain_step(drive_inputs):
    from simpleslam_amd import Frontend, make_register
    d = drive_inputs
    eye = np.tile(np.eye(4), (2, 1, 1))
    fe = Frontend(make_register("loam"))
    got_poses, got_infos = _drive(lambda k, init: fe.stepTimed(d["d_scans"][k], init, eye, [0.0, 0.1], times=d["d_times"], t_ref=0.05), d)
    fe.finish()
    plain = Frontend(make_register("loam"))
    want_poses, want_infos = _drive(lambda k, init: plain.step(d["d_scans"][k], init), d)
    plain.finish()
    for k, (p, q) in enumerate(zip(got_poses, want_poses)):
        np.testing.assert_array_equal(p, q, err_msg=f"pose of scan {k}")
    for k, (a, b) in enumerate(zip(got_infos, want_infos)):
        assert [a[f] for f in INFO] == [b[f] for f in INFO], k
    for i, ((c1, p1), (c2, p2)) in enumerate(zip(_keyframes(fe.map), _keyframes(plain.map))):
        np.testing.assert_array_equal(c1.view(np.uint32), c2.view(np.uint32), err_msg=f"key frame {i}")
        np.testing.assert_array_equal(p1, p2)
    assert got_infos[-1]["keyframes"] >= 2


def test_host_scans_and_refusals(drive_inputs):
    """A host scan with host times gives the device scan's result; a refusal of the deskew comes back under its name and leaves the loop usable; a
    filter queued ahead is dropped."""
    from simpleslam_amd import Frontend, make_register
    from simpleslam_amd.pcr import PcrError
    d = drive_inputs
    fe, fh = Frontend(make_register("loam")), Frontend(make_register("loam"))
    with pytest.raises(PcrError, match="^deskew: .*stamps"):
        fh.stepTimed(d["scans"][0], d["truth"][0], d["motions"][0], [0.0, 0.0, 0.1], times=d["times"], t_ref=0.1)
    with pytest.raises(PcrError, match="0 points"):
        fh.stepTimed(d["scans"][0][:0], d["truth"][0], d["motions"][0], d["stamps"], times=d["times"][:0], t_ref=0.1)
    fh.prefetch(d["d_scans"][1])
    pose_d = pose_h = np.array(d["truth"][0], float)
    for k in range(3):
        pose_d, info_d = fe.stepTimed(d["d_scans"][k], pose_d @ d["cmds"][k], d["motions"][k], d["stamps"], times=d["d_times"], t_ref=0.1)
        pose_h, info_h = fh.stepTimed(d["scans"][k], pose_h @ d["cmds"][k], d["motions"][k], d["stamps"], times=d["times"], t_ref=0.1)
        np.testing.assert_array_equal(pose_d, pose_h, err_msg=f"pose of scan {k}")
        assert [info_d[f] for f in INFO] == [info_h[f] for f in INFO], k
    fe.finish()
    fh.finish()
