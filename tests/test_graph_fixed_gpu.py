"""Fixed poses on the GPU ("Fixed poses"): fixed poses come back bit for bit and the free ones reach graph_fixed_ref's optimum
under both preconditioners and every robust kind, the device's linearisation equals the host's with flags set, the solve's product and its
preconditioners treat a fixed pose's rows and columns as lambda I, an all-fixed graph returns at once, the key-frame store receives the same
bits, and flags that were set and cleared leave no trace."""
import numpy as np
import pytest

import graph_fixed_ref as fr
import graph_fixed_scenes as fs
import graph_ref as gr
import graph_robust_ref as rr
import graph_robust_scenes as rs
from simpleslam_amd import SubMap
from simpleslam_amd.pcr import GRAPH_HOST
# the device against the dense-solve reference after both ran until chi2 stalled: ten times the 2.2e-10 m / 1.2e-11 rad measured there
from test_graph_gpu import BOUND_R, BOUND_T, STALL

pytestmark = pytest.mark.gpu

PRECONDS = ("block_jacobi", "tree")
ROBUST_KINDS = ("huber", "geman_mcclure", "tukey")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _worst(A, B, ids):
    d = [gr.pose_diff(A[p], B[p]) for p in ids]
    return max(x[0] for x in d), max(x[1] for x in d)


def _split(g):
    fixed = sorted(g.fixed)
    return fixed, [p for p in range(len(g.poses)) if p not in g.fixed]


@pytest.fixture(scope="module")
def references():
    """graph_fixed_ref's optimum of every scene and of the robust scene under every kind, computed once: name -> (scene, optimised poses, result)"""
    out = {}
    for name in fs.NAMES:
        g = fs.scenes()[name]
        ref = g.copy()
        res = ref.optimize(rel_tol=0.0, abs_tol=0.0)
        out[name] = (g, ref.poses, res)
    for kind in ROBUST_KINDS:
        g = fs.ring12_false_into_fixed()
        g.kind, g.delta = rr.KINDS[kind], rs.DELTA
        ref = g.copy()
        res = ref.optimize(rel_tol=0.0, abs_tol=0.0)
        out[kind] = (g, ref.poses, res)
    return out


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("name", fs.NAMES)
def test_fixed_poses_stay_and_free_poses_reach_the_reference(name, precond, references):
    g, ref_poses, ref = references[name]
    fixed, free = _split(g)
    pg = fs.to_library(g, 0)
    out = pg.optimize(pcg_preconditioner=precond, **STALL)
    got = pg.poses()
    for p in fixed:
        assert np.array_equal(_bits(got[p]), _bits(g.poses[p])), (name, precond, p)
    dt, dr = _worst(got, ref_poses, free)
    print(f"fixed {name} {precond}: |dt| {dt:.3e} m |dR| {dr:.3e} rad; chi2 {out.chi2_final:.12g} vs {ref['chi2_final']:.12g}; {out}")
    assert dt <= BOUND_T and dr <= BOUND_R, (name, precond, dt, dr)
    assert abs(out.chi2_initial - ref["chi2_initial"]) <= 1e-11 * ref["chi2_initial"]
    assert abs(out.chi2_final - ref["chi2_final"]) <= 1e-9 * ref["chi2_final"] + 1e-12
    assert out.accepted > 0 and out.pcg_iterations > 0 and out.pcg_capped == 0
    moved = [p for p in free if not np.array_equal(got[p], g.poses[p])]
    assert moved == free
    if len(g.poses) - 1 in g.fixed:                       # delta is the identity when the last pose is fixed
        assert np.array_equal(out.delta, np.eye(4))
    else:
        assert np.abs(out.delta - got[-1] @ gr.inv(g.poses[-1])).max() < 1e-12


@pytest.mark.parametrize("kind", ROBUST_KINDS)
def test_a_false_loop_into_a_fixed_pose_under_every_robust_kind(kind, references):
    g, ref_poses, ref = references[kind]
    fixed, free = _split(g)
    for precond in PRECONDS:
        pg = fs.to_library(g, 0)
        out = pg.optimize(pcg_preconditioner=precond, **STALL)
        got = pg.poses()
        for p in fixed:
            assert np.array_equal(_bits(got[p]), _bits(g.poses[p])), (kind, precond, p)
        dt, dr = _worst(got, ref_poses, free)
        s, w, _, _ = pg.betweenWeights()
        print(f"fixed robust {kind} {precond}: |dt| {dt:.3e} m |dR| {dr:.3e} rad; w true {w[11]:.4f} false {w[12]:.3e}; {out}")
        assert dt <= BOUND_T and dr <= BOUND_R, (kind, precond, dt, dr)
        assert out.accepted > 0 and out.pcg_capped == 0
        # robust weights are computed as ever, from s = r^T Omega r: at poses within the bound of the reference's they are the reference's to
        # first order.  |dw| <= max|w'| |ds|; |w'| <= 2/d for all three kinds (Huber 1/(2d) beyond d, Geman-McClure 2 d^2/(d+s)^3, Tukey
        # 2 (1 - s/d)/d); |ds| <= 2 sqrt(s lmax(Omega)) |dr| + lmax |dr|^2; |dr| <= (1 + |t|) B per end, B the pose bound and |t| the longest
        # measured translation (a rotation error swings the other end by that lever), two ends
        s_ref, w_ref = fr.FixedGraph.of(g, g.fixed).between_weights(ref_poses)
        B, d = max(BOUND_T, BOUND_R), rs.DELTA ** 2
        dr_max = 2 * (1 + max(np.linalg.norm(Z[:3, 3]) for _, _, Z, _ in g.betweens)) * B
        lmax = np.array([np.linalg.eigvalsh(Om).max() for _, _, _, Om in g.betweens])
        w_bound = (2 / d) * (2 * np.sqrt(s_ref * lmax) * dr_max + lmax * dr_max ** 2) + 1e-14
        print(f"   weights: worst |dw| {np.abs(w - w_ref).max():.3e}, bound at that factor {w_bound[np.argmax(np.abs(w - w_ref))]:.3e}")
        assert (np.abs(w - w_ref) <= w_bound).all(), (kind, precond, np.abs(w - w_ref), w_bound)


@pytest.mark.parametrize("name", fs.NAMES + ("robust",))
def test_linearize_equals_the_host_bit_for_bit_with_flags_set(name):
    if name == "robust":
        g = fs.ring12_false_into_fixed()
        g.kind, g.delta = rr.TUKEY, rs.DELTA
        g.enabled[4] = False
    else:
        g = fs.scenes()[name]
    dev, host = fs.to_library(g, 0), fs.to_library(g, GRAPH_HOST)
    assert dev.fixed().sum() == len(g.fixed) > 0
    ld, lh = dev.linearize(), host.linearize()
    for what, a, b in zip(("r", "J_from", "J_to"), ld, lh):
        assert np.array_equal(_bits(a), _bits(b)), (name, what, np.abs(a - b).max())
    assert np.float64(ld[3]).view(np.uint64) == np.float64(lh[3]).view(np.uint64), (ld[3], lh[3])
    assert abs(ld[3] - g.chi2()) <= 1e-11 * ld[3]           # chi2 over every factor that is on, between fixed poses or not
    free = fs.to_library(g, 0, fixed=False).linearize()     # ... and the flags change no bit of r, J and chi2
    for what, a, b in zip(("r", "J_from", "J_to", "chi2"), ld, free):
        assert np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b))), (name, what)
    for what, a, b in zip(("s", "w"), dev.betweenWeights()[:2], host.betweenWeights()[:2]):
        assert np.array_equal(_bits(a), _bits(b)), (name, what)


@pytest.mark.parametrize("name", fs.NAMES)
def test_apply_is_lambda_on_fixed_rows_and_the_reduced_product_on_the_rest(name):
    g = fs.scenes()[name]
    fixed, _ = _split(g)
    pg = fs.to_library(g, 0)
    H, _, _, free = g.reduced_equations()
    n = len(g.poses)
    rows = np.array([6 * p + k for p in fixed for k in range(6)])
    x = np.random.default_rng(91).normal(size=6 * n)
    for lam in (0.0, 1e-5, 10.0):
        y = pg.apply(lam, x)
        assert np.array_equal(y[rows], lam * x[rows]), (name, lam)          # exactly lambda x_p
        want = H @ x[free] + lam * x[free]                                  # x of a fixed pose reaches no other row
        err = np.abs(y[free] - want).max() / np.abs(want).max()
        print(f"apply fixed {name} lambda={lam}: relative error {err:.3e}")
        assert err <= 1e-12, (name, lam, err)                               # test_graph_gpu.py's agreement for the plain product


@pytest.mark.parametrize("name", fs.NAMES)
def test_precondition_keeps_fixed_rows_apart(name):
    g = fs.scenes()[name]
    fixed, _ = _split(g)
    pg = fs.to_library(g, 0)
    H, _, _, free = g.reduced_equations()
    n = len(g.poses)
    rows = np.array([6 * p + k for p in fixed for k in range(6)])
    rng = np.random.default_rng(93)
    r = rng.normal(size=6 * n)
    r2 = r.copy()
    r2[rows] = rng.normal(size=rows.size)
    lam = 0.25                                                              # a power of two: r / lambda is exact
    for kind in PRECONDS:
        z, z2 = pg.precondition(lam, r, kind), pg.precondition(lam, r2, kind)
        assert np.array_equal(z[rows], r[rows] / lam) and np.array_equal(z2[rows], r2[rows] / lam), (name, kind)
        assert np.array_equal(_bits(z[free]), _bits(z2[free])), (name, kind)     # r of a fixed pose reaches no free row
    # block Jacobi on the free rows: the inverse of every free pose's diagonal block of the REDUCED H + lambda I
    z = pg.precondition(lam, r, "block_jacobi")
    want = np.concatenate([np.linalg.solve(H[k:k + 6, k:k + 6] + lam * np.eye(6), r[free][k:k + 6]) for k in range(0, free.size, 6)])
    assert np.abs(z[free] - want).max() <= 1e-12 * np.abs(want).max(), name


def test_an_all_fixed_graph_returns_at_once():
    g = fs.scenes()["chain12"]
    pg = fs.to_library(g, 0)
    pg.setFixed(0, len(g.poses))
    for precond in PRECONDS:
        out = pg.optimize(pcg_preconditioner=precond)
        assert (out.iterations, out.accepted, out.pcg_iterations, out.pcg_capped) == (0, 0, 0, 0) and out.converged
        assert out.chi2_initial == out.chi2_final == pg.linearize()[3] > 0 and np.array_equal(out.delta, np.eye(4))
    assert np.array_equal(_bits(pg.poses()), _bits(np.stack(g.poses)))
    pg.setFixed(8, 4, False)                                # something new: real work on the four that were freed
    out = pg.optimize()
    assert out.iterations > 0 and out.accepted > 0 and out.chi2_final < out.chi2_initial
    assert np.array_equal(_bits(pg.poses()[:8]), _bits(np.stack(g.poses[:8])))


def test_the_key_frame_store_gets_the_same_bits_for_fixed_key_frames():
    g = fs.scenes()["g70"]
    fixed, free = _split(g)
    n = len(g.poses)
    rng = np.random.default_rng(95)
    m = SubMap(device=0)
    for k in range(n):
        m.addKeyFrame(rng.normal(size=(8, 4)).astype(np.float32), g.poses[k])
    pg = fs.to_library(g, 0)
    out = pg.optimize()
    assert out.accepted > 0
    pg.applyTo(m)                                           # pcr_map_set_poses_from_graph
    got = pg.poses()
    for p in fixed:
        assert np.array_equal(_bits(m.keyFrame(p)[1]), _bits(g.poses[p])), p
    for p in free:
        assert np.array_equal(_bits(m.keyFrame(p)[1]), _bits(got[p])) and not np.array_equal(got[p], g.poses[p]), p


@pytest.mark.parametrize("precond", PRECONDS)
def test_flags_set_and_cleared_leave_no_trace(precond):
    g = fs.scenes()["eight41"]
    never = fs.to_library(g, 0, fixed=False)
    cleared = fs.to_library(g, 0)
    assert cleared.fixed().any()
    cleared.linearize()                                     # (the device has seen the flags)
    cleared.setFixed(0, len(g.poses), False)
    ra, rb = never.optimize(pcg_preconditioner=precond), cleared.optimize(pcg_preconditioner=precond)
    assert np.array_equal(_bits(never.poses()), _bits(cleared.poses()))
    assert (ra.iterations, ra.accepted, ra.pcg_iterations, ra.chi2_final) == (rb.iterations, rb.accepted, rb.pcg_iterations, rb.chi2_final)
    assert ra.converged and never.optimize(pcg_preconditioner=precond).iterations == 0       # nothing new since a converged run ...
    never.setFixed(3)
    never.setFixed(3, 1, False)                             # ... a flag set and cleared is something new: the early return does not fire
    again = never.optimize(pcg_preconditioner=precond)
    assert again.iterations > 0 and again.converged
