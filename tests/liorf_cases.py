"""The inputs of the liorf tests and the reference's results on them, computed once per process (tests/liorf_ref.py) and shared by the CPU and
the GPU tests.

LINEARIZE: one linearisation.  A 20 000-point map -- the corner scene sampled at ~0.3 m where the scan looks (a 5 x 3 neighbour matrix of
absolute coordinates has a condition number of about sqrt(5) |centroid| / spread, so a patch a few metres from the origin needs that spread to
stay below 100) and a dense slab far away that holds the rest of the points -- and a scan of 2 048 + 37 points drawn from more candidates than
needed: candidates are dropped, on the reference's numbers alone, when they lie within MARGIN_GEN of one of the four gates (the fifth
neighbour's distance, the plane residual, the weight, the tie between the fifth and the sixth neighbour) or when their patch's condition number
exceeds 100.  The candidates include points in empty space (no fifth neighbour within the gate), points at the centres of clusters of five
map points scattered in a 0.7 m cube of free space (five neighbours on no plane: a residual above the threshold) and points a few centimetres
from the sensor, which stands 0.6 m above the ground (a weight below the threshold).

SCENES: the three end-to-end scenes (simpleslam_amd.synth.plane_scene) with their initial guesses.
"""
import functools

import numpy as np

import liorf_ref as R
from simpleslam_amd import synth

N_MAP, N_SCAN = 20000, 2048 + 37
MARGIN, MARGIN_GEN = 1e-3, 2e-3
SCENES = {"corner": dict(seed=1, guess=3), "corridor": dict(seed=1, guess=7), "ground_wall": dict(seed=2, guess=5)}


@functools.lru_cache(maxsize=None)
def linearize_case(seed=0):
    rng = np.random.default_rng([seed, 77])
    n_near = 2400
    cand, near, T = synth.plane_scene("corner", n_map=n_near, n_scan=5000, seed=seed)
    m = np.zeros((N_MAP, 4), np.float32)
    m[:n_near] = near
    nf = N_MAP - n_near
    m[n_near:, 0], m[n_near:, 1], m[n_near:, 2] = rng.uniform(20, 50, nf), rng.uniform(-20, 20, nf), -1.5 + rng.normal(0, 0.01, nf)
    # 18 clusters of five points in free space, each more than a metre from the planes and from each other (a lattice of centres 2 m apart)
    cx, cy, cz = np.meshgrid(np.arange(-1.0, 5.0, 2.0) + 0.2, np.arange(-1.0, 5.0, 2.0) + 0.1, [0.3, 2.0], indexing="ij")
    centres = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], axis=1)
    clusters = centres[:, None, :] + rng.uniform(-0.35, 0.35, (len(centres), 5, 3))
    m[n_near:n_near + 5 * len(centres), :3] = clusters.reshape(-1, 3)
    m = m[rng.permutation(N_MAP)]
    Ti = np.linalg.inv(T)
    extra = []
    extra.append(rng.uniform([-2, -2, 4.5], [4, 4, 6], (40, 3)) @ Ti[:3, :3].T + Ti[:3, 3])          # empty space
    at = np.repeat(centres, 4, axis=0) + rng.uniform(-0.1, 0.1, (4 * len(centres), 3))
    extra.append(at @ Ti[:3, :3].T + Ti[:3, 3])                                                      # inside the clusters
    extra.append(rng.normal(0, 0.01, (40, 3)))                                                       # at the sensor
    ex = np.concatenate(extra)
    ex = np.concatenate([ex, np.zeros((len(ex), 1))], axis=1).astype(np.float32)
    cand = np.concatenate([ex, cand])
    six = R.pose_to_6dof(synth.perturb(T, seed + 3, trans=0.3, rot_deg=3.0))      # all three angles nonzero
    pp = R.per_point(cand, m, R.transformation(six))
    ok = (R.gate_margins(pp) >= MARGIN_GEN).all(axis=1)
    fit = pp["d2"][:, 4].astype(np.float64) < R.DEFAULTS["knn_max_sq"]
    cond = np.zeros(len(cand))
    cond[fit] = R.patch_condition(m, pp["idx"][fit][:, :5])
    ok &= cond <= 100.0
    scan = cand[np.flatnonzero(ok)[:N_SCAN]].copy()
    assert len(scan) == N_SCAN, len(scan)
    scan = scan[rng.permutation(N_SCAN)]
    return dict(scan=scan, map=m, six=six, T_true=T)


@functools.lru_cache(maxsize=None)
def linearize_ref(seed=0):
    """The reference's linearisation of linearize_case at its own float 4x4 (libm's sinf / cosf)"""
    c = linearize_case(seed)
    pp = R.per_point(c["scan"], c["map"], R.transformation(c["six"]), R.row_trig(c["six"]))
    pp["AtA"], pp["AtB"] = R.sums(pp["rows"], pp["coeff"], pp["kept"])
    return pp


@functools.lru_cache(maxsize=None)
def scene(kind):
    s = SCENES[kind]
    scan, m, T = synth.plane_scene(kind, n_map=N_MAP, n_scan=N_SCAN, seed=s["seed"])
    return dict(scan=scan, map=m, T_true=T, T0=synth.perturb(T, s["guess"], trans=0.3, rot_deg=3.0))


@functools.lru_cache(maxsize=None)
def scene_ref(kind):
    c = scene(kind)
    return R.scan2map(c["scan"], c["map"], c["T0"])
