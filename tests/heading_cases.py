"""Registration cases at headings around the full circle, shared by tests/test_heading_cases.py (CPU: every case reaches the branch it
claims and is one the references solve), tests/test_heading_gpu.py (the device against the references) and tests/test_small_math_host.py
(csrc/small_math.h on the CPU, driven with these rotations).

The scene is conftest's world_small recipe -- synth.make_map(30_000, seed=5), synth.make_scan(world, 0, seed=5, beams=16, azimuths=512,
pose=P): 8 192 scan points -- at the position of synth.scan_pose(world, 0, 5) with the rotation Rz(yaw) Ry(pitch) Rx(roll) chosen on
purpose.  What a case's rotation decides:

  t2se3 (csrc/small_math.h)      trace(R) > 0: the quaternion route ("q"); otherwise the largest diagonal entry picks i = 0, 1 or 2.  A
                                 near-level pose has trace 1 + 2 cos(yaw): positive below 120 degrees, i = 2 beyond.
  euler_xyz (csrc/ndt_host.hip)  Matrix3f::eulerAngles(0, 1, 2): atan2f(R12, R22) > 0 flips the first angle by pi ("pi": for a near-level
                                 pose, angles near +-pi), < 0 does not ("zero": angles near 0), == 0 is the boundary ("edge", which takes
                                 the "zero" rule).  Which sign of the 0.01 rad tilt flips depends on the heading: _table().
  liorf's pose_to_6dof           atan2f wraps at yaw = +-180 degrees; roll is about pi when the sensor is upside down.

Two whole-scene cases move map and pose together by a rigid motion G about the map frame's origin (the map re-rounded to float32 once:
both sides of every comparison get the same bytes): G = 179 degrees about x puts t2se3 at i = 0 and liorf's roll at about pi, G = 179
degrees about y puts t2se3 at i = 1.  Both poses are inside every reference's range (liorf's pitch is asinf(-R20): 0.6 and 1.6 degrees
here, nowhere near +-90), so all five methods run them.

Every case is one its references solve from the case's guess (tests/test_heading_cases.py asserts it, none left out).  The guess is
synth.perturb(P, 5, trans=0.2, rot_deg=1.0) as world_small's.  One case stands at synth.scan_pose(world, 1, 5)'s position instead (`position`).
"""
import functools

import numpy as np

from simpleslam_amd import synth

F = np.float32
MAP_POINTS, SEED, BEAMS, AZIMUTHS = 30_000, 5, 16, 512
TILT = 0.01      # rad: synth.scan_pose draws roll and pitch with this standard deviation


def rot_zyx(yaw, pitch, roll):
    """Rz(yaw) Ry(pitch) Rx(roll), as synth.scan_pose builds it"""
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def _case(scene, yaw_deg, tilt, route, family, position=0):
    roll, pitch = {"+-": (TILT, -TILT), "-+": (-TILT, TILT), "level": (0.0, 0.0)}[tilt]
    name = f"{scene}-yaw{yaw_deg:g}-{tilt}"
    return dict(name=name, scene=scene, yaw_deg=float(yaw_deg), roll=roll, pitch=pitch, route=route, family=family, guess=SEED, position=position)


def _table():
    """R12 of Rz Ry Rx is sin(yaw) sin(pitch) cos(roll) - cos(yaw) sin(roll): with roll = -pitch = +-0.01 its sign is that of
    -+(cos(yaw) + sin(yaw)), so which tilt flips depends on the heading -- written out per yaw here, and asserted from R on the CPU"""
    out = []
    # yaw, route, the family of the (+0.01, -0.01) tilt; the (-0.01, +0.01) tilt has the other one
    for yaw, route, fam in ((0, "q", "zero"), (90, "q", "zero"), (-90, "q", "pi"), (119, "q", "zero"),
                            (121, 2, "zero"), (179.9, 2, "pi"), (180, 2, "pi"), (-179.9, 2, "pi")):
        out.append(_case("plain", yaw, "+-", route, fam))
        # (at yaw -179.9 gicp's reference ends 2 to 4 mm from the truth from the guesses of seeds 5 to 10 alike, but its LM loop runs all 64
        #  iterations without meeting the convergence test: the case stands at the position of the drive's next scan, 1.5 m further on)
        out.append(_case("plain", yaw, "-+", route, "pi" if fam == "zero" else "zero", position=1 if yaw == -179.9 else 0))
    for yaw, route in ((0, "q"), (90, "q"), (180, 2)):
        out.append(_case("plain", yaw, "level", route, "edge"))
    # the whole scene turned over: G (Rx or Ry of 179 degrees) applied to the map and to the (+0.01, -0.01) pose at yaw 0.  Both leave
    # atan2f(R12, R22) just above -pi: no flip, and a first angle next to pi all the same
    out.append(_case("rot_x", 0, "+-", 0, "zero"))
    out.append(_case("rot_y", 0, "+-", 1, "zero"))
    return out


CASES = _table()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
# one case of each t2se3 index, for the co-resident LOAM variant
VARIANT_CASES = ["rot_x-yaw0-+-", "rot_y-yaw0-+-", "plain-yaw180-+-"]


def scene_motion(scene):
    """G (3, 3): the rotation about the map frame's origin that the scene's map and poses are moved by"""
    a = np.deg2rad(179.0)
    c, s = np.cos(a), np.sin(a)
    return {"plain": np.eye(3), "rot_x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "rot_y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])}[scene]


@functools.lru_cache(maxsize=None)
def _world():
    world, m = synth.make_map(MAP_POINTS, seed=SEED)
    m.setflags(write=False)
    return world, m


@functools.lru_cache(maxsize=None)
def scene_map(scene):
    """The scene's map, (30 000, 4) float32, read-only: world_small's, moved by the scene's G and rounded to float32 once"""
    _, m = _world()
    if scene == "plain":
        return m
    out = m.copy()
    out[:, :3] = (m[:, :3].astype(np.float64) @ scene_motion(scene).T).astype(F)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, scene, map, scan, truth, init, route, family): the scan is cast in the plain world at the case's pose P and the scene's
    motion G is applied to the map and to P afterwards, so the scan's points do not depend on G"""
    c = BY_NAME[name]
    world, _ = _world()
    P = synth.scan_pose(world, c["position"], SEED)
    P[:3, :3] = rot_zyx(np.deg2rad(c["yaw_deg"]), c["pitch"], c["roll"])
    scan, _ = synth.make_scan(world, 0, seed=SEED, beams=BEAMS, azimuths=AZIMUTHS, pose=P)
    G = np.eye(4)
    G[:3, :3] = scene_motion(c["scene"])
    truth = G @ P
    init = synth.perturb(truth, c["guess"], trans=0.2, rot_deg=1.0)
    out = dict(c, map=scene_map(c["scene"]), scan=scan, truth=truth, init=init)
    for v in (scan, truth, init):
        v.setflags(write=False)
    return out


# ---- the branches, from R alone ---------------------------------------------------------------------------------------------------------
def t2se3_route(R):
    """"q" when trace(R) > 0, else the index of the largest diagonal entry by t2se3's own comparisons (the later entry wins only when larger)"""
    R = np.asarray(R, np.float64)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "q"
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return i


def euler_family(R):
    """"pi" | "zero" | "edge": the sign of atan2f(R12, R22) of the float32 cast of R"""
    Rf = np.asarray(R, np.float64).astype(F)
    r0 = np.arctan2(Rf[1, 2], Rf[2, 2])
    return "pi" if r0 > 0 else ("zero" if r0 < 0 else "edge")


def euler_xyz_f32(R):
    """Matrix3f::eulerAngles(0, 1, 2) of the float32 cast of R, every operation in float32 -> (3,) float32 [roll, pitch, yaw] with
    R = Rx(roll) Ry(pitch) Rz(yaw): the first angle taken into [-pi, 0] before the sign flip of the even permutation."""
    R = np.asarray(R, np.float64).astype(F)
    pi = F(3.14159265358979323846)
    r0 = np.arctan2(R[1, 2], R[2, 2])
    c2 = np.sqrt(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1])
    if r0 > F(0):
        r0 = F(r0 - pi)
        r1 = np.arctan2(-R[0, 2], -c2)
    else:
        r1 = np.arctan2(-R[0, 2], c2)
    s1, c1 = np.sin(r0), np.cos(r0)
    r2 = np.arctan2(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    return np.array([-r0, -r1, -r2], F)


def rot_xyz(e):
    """Rx(e0) Ry(e1) Rz(e2) in float64: what eulerAngles(0, 1, 2) decomposes"""
    e = np.asarray(e, np.float64)
    cx, sx, cy, sy, cz, sz = np.cos(e[0]), np.sin(e[0]), np.cos(e[1]), np.sin(e[1]), np.cos(e[2]), np.sin(e[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def ndt_p6(T):
    """The parameters NDT starts from at the 4x4 pose T: [t; eulerAngles(0, 1, 2)] of its Matrix4f cast, as float64"""
    Tf = np.asarray(T, np.float64).astype(F)
    return np.concatenate([Tf[:3, 3], euler_xyz_f32(Tf[:3, :3])]).astype(np.float64)


# ---- the references' own results ----------------------------------------------------------------------------------------------------------
METHODS = ["loam", "vgicp", "gicp", "ndt", "liorf"]
# NDT: world_small's map has a point every 0.5 m, four to a square metre of wall or ground, and a voxel needs six points: at the default
# 1 m resolution the reference builds next to no Gaussian and "converges" without a step.  3 m voxels hold about forty points each; the
# reference then takes three or four Newton steps from every case's guess.  (tests/test_ndt_gpu.py varies the resolution the same way.)
NDT_RESOLUTION = 3.0
# gicp's and liorf's references are numpy (tests/gicp_ref.py, tests/liorf_ref.py: a brute-force search and a Python loop over the points),
# about 3 s and 1.3 s per pass and thousand points here.  They get every fourth point of the scan -- 2 048 points, the size of liorf's own
# tests -- and so does the device in every comparison with them: same headings, same map, a quarter of the time.
PY_REF_STRIDE = 4
# "Found the truth", as each method's GPU test file puts it: tests/test_loam_gpu.py:73-74, tests/test_vgicp_gpu.py:111-112,
# tests/test_gicp_gpu.py:271, tests/test_liorf_gpu.py:269.  tests/test_ndt_gpu.py has none, and tests/test_fullsize_vgicp_ndt_gpu.py says
# why: NDT stops as soon as a step is shorter than its transformation epsilon of 0.1.  That epsilon is what its stop rule resolves, so it
# is the bound here, for the translation and the rotation alike (the step's norm covers all six parameters).
TRUTH_BOUND = dict(loam=(0.02, 2e-3), vgicp=(0.05, 5e-3), gicp=(0.05, 5e-3), liorf=(0.03, float(np.radians(0.3))), ndt=(0.1, 0.1))
GOLDEN = "heading_refs.npz"      # under tests/golden: the two numpy references' alignments, recorded (tests/test_heading_cases.py holds them to a fresh run)


def method_scan(method, c):
    """The scan a method's comparisons use, on both sides"""
    return np.ascontiguousarray(c["scan"][::PY_REF_STRIDE]) if method in ("gicp", "liorf") else c["scan"]


@functools.lru_cache(maxsize=None)
def gicp_covariances(name):
    """(C_A of the case's gicp scan, C_B of its map): the oracle's, as tests/gicp_ref.world_small_case takes them"""
    import oracle
    c = case(name)
    CA = oracle.vgicp_covariances(method_scan("gicp", c), threads=8)
    CB = _map_covariances(c["scene"])
    CA.setflags(write=False)
    return CA, CB


@functools.lru_cache(maxsize=None)
def _map_covariances(scene):
    import oracle
    CB = oracle.vgicp_covariances(scene_map(scene), threads=8)
    CB.setflags(write=False)
    return CB


@functools.lru_cache(maxsize=None)
def reference(method, name):
    """The reference's alignment from the case's guess, computed here -> dict(pose, converged, iterations[, n]) (n: LOAM's per-iteration count)"""
    import oracle
    c = case(name)
    scan = method_scan(method, c)
    if method == "loam":
        po, co, info = oracle.loam_scan2map(scan, c["map"], c["init"], trace=True)
        return dict(pose=po, converged=co, iterations=info["iters_run"], n=info["n"][: info["iters_run"]])
    if method == "vgicp":
        po, co, info = oracle.vgicp_scan2map(scan, c["map"], c["init"], oracle.vgicp_params(threads=8))
        return dict(pose=po, converged=co, iterations=info["outer"])
    if method == "ndt":
        po, co, info = oracle.ndt_scan2map(scan, c["map"], c["init"], oracle.ndt_params(resolution=NDT_RESOLUTION))
        return dict(pose=po, converged=co, iterations=info["iterations"])
    if method == "gicp":
        import gicp_ref
        CA, CB = gicp_covariances(name)
        a = gicp_ref.align(scan, c["map"], c["init"], CA, CB)
        return dict(pose=a["pose"], converged=a["converged"], iterations=a["outer"])
    if method == "liorf":
        import liorf_ref
        r = liorf_ref.scan2map(scan, c["map"], c["init"])
        return dict(pose=r["pose"], converged=r["converged"], iterations=r["iterations"])
    raise KeyError(method)


@functools.lru_cache(maxsize=None)
def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))


def recorded_reference(method, name):
    """gicp's and liorf's reference() as recorded under tests/golden (they take seconds per case); the three C oracles are run afresh"""
    if method not in ("gicp", "liorf"):
        return reference(method, name)
    g = _golden()
    k = [str(s) for s in g["names"]].index(name)
    return dict(pose=g[method + "_pose"][k].copy(), converged=bool(g[method + "_converged"][k]), iterations=int(g[method + "_iterations"][k]))


def record_golden(path):
    """Writes the golden file from a fresh run of the two numpy references over every case"""
    out = dict(names=np.array(NAMES))
    for m in ("gicp", "liorf"):
        refs = [reference(m, n) for n in NAMES]
        out[m + "_pose"] = np.stack([r["pose"] for r in refs])
        out[m + "_converged"] = np.array([r["converged"] for r in refs])
        out[m + "_iterations"] = np.array([r["iterations"] for r in refs], np.int32)
    np.savez_compressed(path, **out)
