"""CPU tests: the f32 oracle and the f64 restatement under rolled, pitched and translated cameras (tests/poses.py).

Every other camera of the suite is a yaw about +y, under which a view matrix read transposed in viewmatrix[1] / [4] /
[6] / [9] is bit-identical to the right one.  Here: the pose table itself; the oracle against ref64 on every pose at
the unchanged bars; rigid invariance of both (a frame of camera (R, T) equals the frame of the origin camera over the
scene moved by the inverse pose -- no reference needed, so ref64 and the oracle cannot share a misreading of the
matrix layout); ref64's gradcheck under a dense view matrix; and how far from the origin f32 reaches (DESIGN.md
section 2), which fixes the distance the GPU comparisons with f64 may use (tests/test_gpu_poses.py)."""
import numpy as np
import pytest
import torch

import poses as PZ
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import grad_close, masked_upstream
from oracle import oracle as O
from poses import POSES, PURE, WITHIN_REACH, posed
from test_ref64 import _gradcheck_and_split_chain_rule, _gradcheck_scene, _oracle_vs_f64

MAIN = (1500, 200, 120, 13, 3)
SCENES = {"P1500_D3": MAIN, "P7_D1": (7, 33, 17, 3, 1)}
# the (2 500, 257 x 131) scene of tests/test_gpu_poses.py under the pose it is rendered with there
BIG, BIG_POSE = (2500, 257, 131, 4, 2), "rpy"


def test_pose_table():
    assert set(PURE) < set(POSES) and {"roll90", "pitch+35", "pitch-35", "rpy", "zup", "behind", "far"} <= set(POSES)
    for name, (Rcw, T) in POSES.items():
        assert Rcw.dtype == np.float64 and T.dtype == np.float64
        assert np.abs(Rcw @ Rcw.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rcw) - 1.0) <= 1e-15, name
        v = PZ.camera(200, 120, Rcw, T)["viewmatrix"].ravel()
        if name not in PURE:  # the point of the exercise: the transposed reading differs
            assert v[1] != v[4] and v[6] != v[9] and v[1] and v[4] and v[6] and v[9], name
    assert np.abs(POSES["rpy"][0]).min() >= 0.1
    Rz = POSES["zup"][0]  # optical axis along world +x, image up along world +z, tilted a few degrees
    c10, c1 = np.cos(np.radians(10.0)), np.cos(np.radians(1.0))
    assert c10 < Rz[:, 2] @ [1.0, 0, 0] < c1 and c10 < -Rz[:, 1] @ [0, 0, 1.0] < c1 and c10 < -Rz[:, 0] @ [0, 1.0, 0] < c1
    assert np.array_equal(POSES["behind"][0], np.diag([-1.0, 1.0, -1.0]))
    dist = {k: float(np.linalg.norm(T)) for k, (_, T) in POSES.items()}
    assert min(dist.values()) == 0.0 and any(1.0 < d < 6.0 for d in dist.values())
    assert dist["zup"] == pytest.approx(PZ.REACH, rel=1e-15) and 200.0 < dist["far"] < 500.0
    assert all(dist[k] <= PZ.REACH * (1 + 1e-15) for k in WITHIN_REACH)


def test_camera_is_make_camera_generalised():
    """poses.camera from make_camera's own R and T is make_camera, bit for bit; the identity pose leaves a scene
    untouched; a posed scene differs from its base in the means and the three camera arrays only."""
    for yaw, pos in ((0.0, (0.0, 0.0, 0.0)), (17.0, (0.3, -0.2, 0.4)), (-21.0, (0.0, 0.0, 0.0)), (140.0, (3.5, -1.25, 0.75))):
        a = np.radians(yaw)
        Rcw = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        want, got = S.make_camera(257, 131, yaw_deg=yaw, position=pos), PZ.camera(257, 131, Rcw, pos)
        assert want.keys() == got.keys()
        for k in want:
            assert np.array_equal(want[k], got[k]) and np.asarray(want[k]).dtype == np.asarray(got[k]).dtype, (yaw, k)
    sc = S.make_scene(300, 70, 50, 11, sh_degree=3)
    same = posed(sc, np.eye(3), np.zeros(3))
    moved = posed(sc, *POSES["rpy"])
    for k in sc:
        assert np.array_equal(sc[k], same[k]) if sc[k] is not None else same[k] is None, k
        if k not in ("means3D", "viewmatrix", "projmatrix", "campos"):
            assert moved[k] is sc[k] or moved[k] == sc[k], k
    assert moved["means3D"].dtype == np.float32
    # the camera sees the moved means where the origin camera saw the base ones
    t = moved["means3D"].astype(np.float64) @ moved["viewmatrix"][:3, :3] + moved["viewmatrix"][3, :3]
    assert np.abs(t - sc["means3D"]).max() <= 2e-5
    assert np.abs(moved["campos"] - POSES["rpy"][1]).max() <= 1e-6


def _ratios(sc, seed):
    fr, r, g = _oracle_vs_f64(sc, seed)   # asserts the unchanged bars and the fragile cap of 0.5 %
    w = PZ.ratios_against_ref64(fr, r, g)
    print("oracle worst |d| / bar against f64: %.3f (%s)" % (max(w.values()), max(w, key=w.get)),
          {k: round(v, 3) for k, v in w.items()})
    return w


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("pose", WITHIN_REACH)
def test_oracle_matches_f64_posed(pose, scene):
    """The oracle inside the f64 bars on every pose within reach, and at <= 0.5 of each: the headroom the GPU
    comparisons of tests/test_gpu_poses.py are entitled to."""
    P, W, H, seed, D = SCENES[scene]
    w = _ratios(posed(S.make_scene(P, W, H, seed, sh_degree=D), *POSES[pose]), seed)
    assert max(w.values()) <= 0.5, w


def test_oracle_matches_f64_posed_big():
    P, W, H, seed, D = BIG
    w = _ratios(posed(S.make_scene(P, W, H, seed, sh_degree=D), *POSES[BIG_POSE]), seed)
    assert max(w.values()) <= 0.5, w


@pytest.mark.parametrize("pose", ["rpy", "zup"])
@pytest.mark.parametrize("kind", ["cov3D_precomp", "jacobian_clamp", "sh_clamp", "scale_modifier"])
def test_oracle_matches_f64_paths_posed(kind, pose):
    sc, seed = PZ.posed_path_scene(kind, *POSES[pose])
    fr, r, g = _oracle_vs_f64(sc, seed)
    vis = fr.radii > 0
    if kind == "cov3D_precomp":   # (the same side conditions as tests/test_ref64.py: the path is really taken)
        assert np.abs(r["dL_dcov3D"]).max() > 0 and not g["dL_dscales"].any()
    elif kind == "jacobian_clamp":
        out = np.zeros(fr.P, bool)
        out[vis] = R.beyond_jacobian_clamp(sc, np.flatnonzero(vis)).numpy()
        assert out.sum() >= 10 and (np.abs(r["dL_dconic"][out]).max(axis=(1, 2)) > 0).sum() >= 10
    elif kind == "sh_clamp":
        cl = fr.clamped.astype(bool) & vis[:, None]
        assert cl.sum() >= 100 and not r["dL_dsh"].transpose(0, 2, 1)[cl].any()


def _rigid_pair(kind, Rcw, T, dtype):
    """(posed scene A, origin scene B) of one world: B is A moved by the inverse pose.  Means of both from the same
    f64 world positions, each rounded once (not at all for dtype f64); B's quaternions are A's left-multiplied by the
    quaternion of R_cw^T; cameras in `dtype`."""
    P, W, H, seed = 1500, 200, 120, 21
    base = S.make_scene(P, W, H, seed, sh_degree=0)
    if kind == "colors_precomp":
        base["colors_precomp"] = np.random.default_rng(seed).uniform(0, 1, (P, 3)).astype(np.float32)
        base["shs"] = None
    world = base["means3D"].astype(np.float64) @ Rcw.T + T          # the world's f64 truth
    # ... and unit quaternions in f64: the rasterizer takes a quaternion as given (forward.cu:146), and its matrix is a
    # rotation -- so that the product of two is the matrix of the quaternion product -- only for a unit one
    q = base["rotations"].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    A = dict(base, **PZ.camera(W, H, Rcw, T, dtype=dtype), means3D=world.astype(dtype), rotations=q.astype(dtype))
    B = dict(base, **PZ.camera(W, H, np.eye(3), np.zeros(3), dtype=dtype), means3D=((world - T) @ Rcw).astype(dtype),
             rotations=PZ.quat_mul(PZ.quat_of(Rcw.T), q).astype(dtype))
    return A, B, seed


def _rigid_frames(pose, kind):
    Rcw, T = POSES[pose]
    A, B, seed = _rigid_pair(kind, Rcw, T, np.float32)
    O.set_threads(1)
    fa, fb = O.forward(A), O.forward(B)
    ok = (fa.fragile == 0) & (fb.fragile == 0)
    assert (~ok).mean() < 5e-3
    dcol, dacc = masked_upstream(200, 120, seed, (~ok).astype(np.uint8))
    colour = "dL_dcolors" if kind == "colors_precomp" else "dL_dsh"
    return A, B, fa, fb, ok, dcol, dacc, ("dL_dmeans3D", "dL_dscales", "dL_dopacity", colour)


@pytest.mark.parametrize("kind", ["sh0", "colors_precomp"])
@pytest.mark.parametrize("pose", WITHIN_REACH)
def test_rigid_invariance_ref64(pose, kind):
    """Camera (R_cw, T) over a scene = the origin camera over the scene moved by the inverse pose.  In ref64, with f64
    cameras and one discrete structure for both frames: images to 1e-11, dL_dmeans3D mapped by R_cw^T and the scale,
    opacity and colour gradients equal to 1e-9 of the row."""
    Rcw, T = POSES[pose]
    _, _, _, fb, _, dcol, dacc, names = _rigid_frames(pose, kind)
    A, B, _ = _rigid_pair(kind, Rcw, T, np.float64)
    ra, rb = R.render(A, fb, dcol, dacc), R.render(B, fb, dcol, dacc)
    for k in ("out_color", "out_depth", "out_acc"):
        assert np.abs(ra[k] - rb[k]).max() <= 1e-11, (k, float(np.abs(ra[k] - rb[k]).max()))
    ra["dL_dmeans3D"] = ra["dL_dmeans3D"] @ Rcw
    for k in names:
        rows = np.abs(rb[k]).reshape(fb.P, -1).max(1)
        err = np.abs(ra[k] - rb[k]).reshape(fb.P, -1).max(1)
        assert rows.max() > 0 and (err <= 1e-9 * rows).all(), (k, float((err / np.maximum(rows, 1e-300)).max()))


@pytest.mark.parametrize("kind", ["sh0", "colors_precomp"])
@pytest.mark.parametrize("pose", WITHIN_REACH)
def test_rigid_invariance_oracle(pose, kind):
    """The same two frames in the f32 oracle, each on its own discrete structure and its own once-rounded means:
    images to 1e-4 off both fragile maps, gradients to grad_close's bound with its `slack` term for both frames.

    The two backwards are handed different 2-D values: each frame's means2D / conic / colour are that frame's f32
    evaluation of its own rounded means (at 10 m a mean moves by up to 5e-7 m in rounding, 3e-5 px for a near splat
    of ~1 px sigma).  grad_close's plain bound is for two f32 backwards fed the SAME 2-D values; where they differ,
    its `slack` term says how far the exact gradient moves between the exact 2-D values and the ones a frame was
    handed (ref64.render(..., slack=True)).  Here the exact values are those of the f64 world, unrounded, which
    test_rigid_invariance_ref64 shows to be the same for both frames; each frame adds its own slack against them.
    (A row of A's means slack is bounded by its Euclidean norm after the rotation.)  Measured worst |d| / bound:
    0.70 (zup, dL_dscales; 2.4 against the plain bound: one near splat whose dL_dconic moves by 1.2e-4 relative
    under the input rounding, amplified by the conic -> cov chain), <= 0.4 elsewhere."""
    Rcw, T = POSES[pose]
    A, B, fa, fb, ok, dcol, dacc, names = _rigid_frames(pose, kind)
    for k in ("out_color", "out_depth", "out_acc"):
        scale = max(1.0, float(np.abs(getattr(fb, k)).max())) if k == "out_depth" else 1.0
        err = np.abs(getattr(fa, k) - getattr(fb, k)).max(0)
        assert err[ok].max() <= 1e-4 * scale, (k, float(err[ok].max()))
    ga, gb = O.backward(fa, A, dcol, dacc), O.backward(fb, B, dcol, dacc)
    ga["dL_dmeans3D"] = (ga["dL_dmeans3D"].astype(np.float64) @ Rcw).astype(np.float32)
    A64, B64, _ = _rigid_pair(kind, Rcw, T, np.float64)
    sa = R.render(A64, fa, dcol, dacc, slack=True)["slack"]
    sb = R.render(B64, fb, dcol, dacc, slack=True)["slack"]
    sa["dL_dmeans3D"] = np.repeat(np.linalg.norm(sa["dL_dmeans3D"], axis=1, keepdims=True), 3, 1)
    for k in names:
        assert np.abs(gb[k]).max() > 0
        grad_close(ga[k], gb[k], k, slack=sa[k].reshape(fb.P, -1).max(1) + sb[k].reshape(fb.P, -1).max(1))


def test_autograd_matches_finite_differences_under_a_dense_view_matrix():
    """gradcheck of the whole restated forward as in tests/test_ref64.py (same eps, atol, rtol, same "no pixel near a
    cut" precondition), the five splats seen by the rpy camera at a nonzero T."""
    Rcw, T = POSES["rpy"]
    assert np.abs(T).min() > 0
    _gradcheck_and_split_chain_rule(posed(_gradcheck_scene(), Rcw, T))


def _reach_table():
    P, W, H, seed, D = MAIN
    base = S.make_scene(P, W, H, seed, sh_degree=D)
    rows = {}
    for d in PZ.REACH_DISTANCES:
        sc = posed(base, PZ.ZUP_TILTED, d * PZ.REACH_DIR)
        O.set_threads(1)
        fr = O.forward(sc)
        dcol, dacc = masked_upstream(W, H, seed, fr.fragile)
        rows[d] = PZ.ratios_against_ref64(fr, R.render(sc, fr, dcol, dacc, slack=True), O.backward(fr, sc, dcol, dacc))
    return rows


def test_how_far_float32_reaches():
    """The oracle's worst error / bar against f64 per image and gradient group, camera under the zup attitude at
    |T| = 0 ... 300 m along poses.REACH_DIR (the table of DESIGN.md section 2; printed).  poses.REACH, the distance of
    the `zup` pose and the largest any f64 comparison on the GPU uses, is the largest of the table at which the oracle
    alone stays at <= 0.5 of every bar."""
    rows = _reach_table()
    for d, w in rows.items():
        print("|T| = %5.0f m  worst %.3f (%s) " % (d, max(w.values()), max(w, key=w.get)),
              {k: round(v, 3) for k, v in w.items()})
    assert PZ.REACH in rows and max(rows[PZ.REACH].values()) <= 0.5, rows[PZ.REACH]
    beyond = [d for d in rows if d > PZ.REACH]
    assert all(max(rows[d].values()) > 0.5 for d in beyond), "poses.REACH is not the largest distance within 0.5"


def test_far_pose_error_is_input_rounding():
    """At the `far` pose (|T| = 341 m) the oracle's images leave the 1e-4 bar.  That is the reach of f32, not an error
    of the oracle: W m + t cancels coordinates of hundreds of metres to a few, so the view-space position carries the
    rounding of |m|.  ref64 itself, evaluated at means displaced by half an ulp of |m| along one world axis, moves by
    at least as much as the oracle is away from it (worst axis and sign of the six)."""
    P, W, H, seed, D = MAIN
    sc = posed(S.make_scene(P, W, H, seed, sh_degree=D), *POSES["far"])
    O.set_threads(1)
    fr = O.forward(sc)
    ok = fr.fragile == 0
    r0 = R.render(sc, fr)
    half_ulp = 0.5 * np.spacing(np.float32(np.linalg.norm(sc["means3D"], axis=1).max())).astype(np.float64)
    for k in ("out_color", "out_acc"):
        off = float(np.abs(getattr(fr, k).astype(np.float64) - r0[k]).max(0)[ok].max())
        moved = 0.0
        for axis in range(3):
            for sign in (-1.0, 1.0):
                m = sc["means3D"].astype(np.float64)
                m[:, axis] += sign * half_ulp
                moved = max(moved, float(np.abs(R.render(dict(sc, means3D=m), fr)[k] - r0[k]).max(0)[ok].max()))
        print("%s: oracle %.3e from f64; f64 moves %.3e under half an ulp (%.2e m) of |m|" % (k, off, moved, half_ulp))
        assert off > 1e-4, "the far pose is within the fixed bar: compare it with f64 like the others"
        assert moved >= off, (k, off, moved)
