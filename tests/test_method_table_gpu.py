"""What the C ABI's dispatch layer decides per method (loam, ndt, vgicp, gicp, liorf), pinned entry point by entry point: when a handle
has a target, when pcr_scan2map_submap rebuilds one, which parameters a prepared target is derived from, what pcr_fitness answers, who
refuses a sharded target and in which words.  Every expectation is what the library did before its method table existed (recorded on the
commit before it, where this file passes unchanged).  One tiny scene: three planes, a target of 8 000 points, a scan of 2 000, 16-byte rows."""
import numpy as np
import pytest

from simpleslam_amd import PcrError, SubMap, make_register, synth

pytestmark = pytest.mark.gpu

METHODS = ["loam", "ndt", "vgicp", "gicp", "liorf"]
# the parameters a method's prepared target is derived from (pcr_set_params drops the target when one changes) ...
OWN = {
    "loam": [("loam_knn_max_sq", 4.0)],
    "ndt": [("ndt_resolution", 2.0)],
    "vgicp": [("vgicp_resolution", 2.0), ("vgicp_voxel_mode", 1)],
    "gicp": [("vgicp_resolution", 2.0), ("vgicp_regularization", 0)],
    "liorf": [],
}
# ... and parameters that shape another method's target: the handle's own stays
OTHERS = {
    "loam": [("ndt_resolution", 2.0), ("vgicp_resolution", 2.0), ("vgicp_voxel_mode", 1), ("vgicp_regularization", 0)],
    "ndt": [("loam_knn_max_sq", 4.0), ("vgicp_resolution", 2.0), ("vgicp_voxel_mode", 1), ("vgicp_regularization", 0)],
    "vgicp": [("loam_knn_max_sq", 4.0), ("ndt_resolution", 2.0)],
    "gicp": [("loam_knn_max_sq", 4.0), ("ndt_resolution", 2.0), ("vgicp_voxel_mode", 1)],
    "liorf": [("loam_knn_max_sq", 4.0), ("ndt_resolution", 2.0), ("vgicp_resolution", 2.0), ("vgicp_voxel_mode", 1), ("vgicp_regularization", 0)],
}
# liorf's getFitnessScore() of this scene after scan2Map from the guess below, as the commit before the method table returns it.  Compared to
# 1e-9: the mean of 2 000 squared distances summed in f64 in whatever order is within 2000 * 2^-53 = 2e-13 of it
LIORF_FITNESS = 0.003712913365326358


@pytest.fixture(scope="module")
def scene(gpu):
    scan, m, T = synth.plane_scene("corner", n_map=8000, n_scan=2000, seed=3)
    guess = T.copy()
    guess[:3, 3] += [0.05, -0.04, 0.03]
    assert scan.strides[0] == 16 and m.strides[0] == 16
    return dict(scan=scan, map=m, guess=guess)


@pytest.fixture
def reg(request, gpu):
    r = make_register(request.param)
    yield r
    r.close()


def by_method(f):
    return pytest.mark.parametrize("reg", METHODS, indirect=True)(f)


def aligned(reg, scene):
    pose = scene["guess"].copy()
    reg.align(scene["scan"], pose)
    return pose


@by_method
def test_a_target_stands_from_set_target_to_invalidate(reg, scene):
    with pytest.raises(PcrError, match="no target"):
        aligned(reg, scene)
    reg.setTarget(scene["map"])
    first = aligned(reg, scene)
    assert np.isfinite(first).all()
    np.testing.assert_array_equal(aligned(reg, scene), first)
    reg.invalidateTarget()
    with pytest.raises(PcrError, match="no target"):
        aligned(reg, scene)


@by_method
def test_a_submap_generation_is_prepared_once(reg, scene):
    sm = SubMap()
    sm.addKeyFrame(scene["map"], np.eye(4))
    assert sm.updateMap(np.zeros(3), radius=8.0, grid_size=0.1) > 4000
    builds = lambda: reg.stats()["target_builds"]
    before = builds()
    p1, p2 = scene["guess"].copy(), scene["guess"].copy()
    reg.scan2MapSubmap(scene["scan"], sm, p1)
    reg.scan2MapSubmap(scene["scan"], sm, p2)
    np.testing.assert_array_equal(p1, p2)
    assert builds() == before + 1
    reg.invalidateTarget()
    p3 = scene["guess"].copy()
    reg.scan2MapSubmap(scene["scan"], sm, p3)
    np.testing.assert_array_equal(p3, p1)
    assert builds() == before + 2


@by_method
def test_a_changed_parameter_drops_the_target_derived_from_it(reg, scene):
    for name, value in OWN[reg.method]:
        reg.setTarget(scene["map"])
        aligned(reg, scene)
        reg.set_params(**{name: value})
        with pytest.raises(PcrError, match="no target"):
            aligned(reg, scene)


@by_method
def test_another_methods_parameter_leaves_the_target_standing(reg, scene):
    reg.setTarget(scene["map"])
    first = aligned(reg, scene)
    for name, value in OTHERS[reg.method]:
        reg.set_params(**{name: value})
        np.testing.assert_array_equal(aligned(reg, scene), first, err_msg=name)


@by_method
def test_fitness_score_after_scan2map(reg, scene):
    pose = scene["guess"].copy()
    reg.scan2Map(scene["scan"], scene["map"], pose)
    score = reg.getFitnessScore()
    print(reg.method, "fitness", repr(score))
    if reg.method in ("loam", "ndt"):
        assert score == 0.0
    elif reg.method == "liorf":
        assert score == pytest.approx(LIORF_FITNESS, rel=1e-9)
    else:
        assert np.isfinite(score) and 0.0 < score < 1e300
    assert reg.getFitnessScore() == score
    if reg.method == "liorf":      # its score counts the points within 1 m of the target, and is -1 when none is: a guess 50 m above the scene
        far = scene["guess"].copy()
        far[2, 3] += 50.0
        reg.scan2Map(scene["scan"], scene["map"], far)
        assert reg.getFitnessScore() == -1.0


@pytest.mark.parametrize("reg", ["gicp", "liorf"], indirect=True)
def test_unshardable_methods_refuse_at_every_entry_point(reg, scene):
    lo, hi = [-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]
    calls = {
        "pcr_set_query_tile": lambda: reg.set_query_tile(lo, hi),
        "pcr_set_shard": lambda: reg.set_shard(lo, hi, 2.0),
        "pcr_comm_init_host": lambda: reg.comm_init_host(lambda ptr, count, op, user: 0, 0, 1),
        "pcr_comm_init_peer": lambda: reg.comm_init_peer([bytes(64)], 0, 1),
        "pcr_comm_init": lambda: reg.comm_init(bytes(128), 0, 1),
    }
    for entry, call in calls.items():
        with pytest.raises(PcrError) as e:
            call()
        assert str(e.value) == f"{reg.method}: sharded targets are not supported in this version ({entry})"
    # clearing a tile or a collective that was never set is no sharding: it succeeds, before the refusal
    reg.set_query_tile([1.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    reg.set_shard([1.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0)
    reg.comm_init_host(None, 0, 1)
    reg.setTarget(scene["map"])
    assert np.isfinite(aligned(reg, scene)).all()


@pytest.mark.parametrize("reg, bound, rebuilds", [("loam", 8.0, 0), ("ndt", 8.0, 0), ("vgicp", 7.5, 1)], indirect=["reg"])
def test_set_shard_drops_the_prepared_target_of_vgicp_alone(reg, bound, rebuilds, scene):
    """pcr_set_shard drops the voxels of a vgicp handle (they were checked against another halo); a loam or ndt handle keeps what it has."""
    sm = SubMap()
    sm.addKeyFrame(scene["map"], np.eye(4))
    sm.updateMap(np.zeros(3), radius=8.0, grid_size=0.1)
    first = scene["guess"].copy()
    reg.scan2MapSubmap(scene["scan"], sm, first)
    builds = reg.stats()["target_builds"]
    reg.set_shard([-bound] * 3, [bound] * 3, 2.0)
    reg.set_shard([1.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0)      # (an empty tile: the handle is whole again)
    if rebuilds:
        with pytest.raises(PcrError, match="no target"):
            aligned(reg, scene)
    else:
        aligned(reg, scene)
    again = scene["guess"].copy()
    reg.scan2MapSubmap(scene["scan"], sm, again)
    np.testing.assert_array_equal(again, first)
    assert reg.stats()["target_builds"] == builds + rebuilds
