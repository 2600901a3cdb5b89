"""CPU tests: the f32 oracle and the f64 restatement under cameras whose focal lengths differ (tests/intrinsics.py).

Every other camera of the suite has square pixels, under which focal_x and focal_y are the same float and a rasterizer
that reads one for the other is bit-identical to the right one.  Here: the table itself; a closed form of the EWA
projection of one isotropic Gaussian that neither ref64 nor the oracle wrote, so that the two cannot share a misreading
of which focal length goes where; the oracle against ref64 on every entry and on three paths at the unchanged bars, at
<= 0.5 of each (the headroom the GPU comparisons of tests/test_gpu_intrinsics.py are entitled to); ref64's gradcheck with
fx != fy under a dense view matrix; and the blind spot as a fact: an oracle that reads focal_x for focal_y is rejected
by ref64 on every entry, the reference's own 0.4 % included, and is invisible on the suite's main square-pixel scene."""
import math

import numpy as np
import pytest
import torch

import intrinsics as IZ
import poses as PZ
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, check_against_ref64, masked_upstream
from intrinsics import INTRINSICS
from oracle import oracle as O
from test_ref64 import IMAGES, _gradcheck_and_split_chain_rule, _gradcheck_scene, _oracle_vs_f64

U = 2.0 ** -24          # unit roundoff of f32


def _focals_as_the_kernels_compute_them(sc):
    """api.hip make_params / gsr_oracle.c: W / (2.0f * tan_fovx), H / (2.0f * tan_fovy), in f32."""
    two = np.float32(2.0)
    return (np.float32(sc["W"]) / (two * np.float32(sc["tanfovx"])),
            np.float32(sc["H"]) / (two * np.float32(sc["tanfovy"])))


# ------------------------------------------------- the table -------------------------------------------------
def test_reference_calibrations_all_have_two_focal_lengths():
    cal = IZ.reference_calibrations()
    assert len(cal) == 5 and all(c["fx"] != c["fy"] for c in cal.values())
    W, H, fx, fy, pose, spec = INTRINSICS["ntu/4"]
    assert (W, H) == (188, 120) and pose is None
    assert fx == pytest.approx(106.256475, rel=1e-12) and fy == pytest.approx(106.6994, rel=1e-12)
    assert 0.003 < fy / fx - 1.0 < 0.005          # the realistic case: 0.4 %


def test_intrinsics_table():
    assert set(INTRINSICS) == {"ntu/4", "wide_y", "tall_y", "tiny", "big"}
    for name in INTRINSICS:
        W, H, fx, fy, pose, (P, seed, D) = INTRINSICS[name]
        sc, _ = IZ.entry(name)
        kx, ky = _focals_as_the_kernels_compute_them(sc)
        assert kx != ky and abs(float(ky) / float(kx) - 1.0) >= 3e-3, name
        assert float(kx) == pytest.approx(fx, rel=4 * U) and float(ky) == pytest.approx(fy, rel=4 * U), name
        assert abs(sc["tanfovy"] / sc["tanfovx"] / (H / W) - 1.0) >= 3e-3, name
        assert sc["means3D"].shape == (P, 3) and sc["means3D"].dtype == np.float32 and sc["sh_degree"] == D
        assert np.array_equal(sc["bg"], np.asarray(IZ.BG, np.float32))
        assert (pose is None) == np.array_equal(sc["viewmatrix"], np.eye(4, dtype=np.float32)), name
    assert {INTRINSICS[k][4] for k in INTRINSICS} >= {None, "rpy", "zup"}
    # the splats fill the anisotropic frustum: their view-space spread over z follows the two tangents
    sc, _ = IZ.entry("wide_y")
    m = sc["means3D"][sc["means3D"][:, 2] > 1.0].astype(np.float64)
    assert 0.95 * 1.1 * sc["tanfovx"] < np.abs(m[:, 0] / m[:, 2]).max() <= 1.1 * sc["tanfovx"] * (1 + 1e-6)
    assert 0.95 * 1.1 * sc["tanfovy"] < np.abs(m[:, 1] / m[:, 2]).max() <= 1.1 * sc["tanfovy"] * (1 + 1e-6)


@pytest.mark.parametrize("W,H", [(200, 120), (33, 17), (257, 131), (70, 50), (160, 96), (640, 480)])
def test_camera_with_square_pixels_is_make_camera(W, H):
    """intrinsics.camera with fy = fx is poses.camera, and from make_camera's own R and T it is make_camera, bit for
    bit: the new cameras differ from the old ones in the two focal lengths only."""
    fx = IZ.square_fx(W)
    for yaw, pos in ((0.0, (0.0, 0.0, 0.0)), (17.0, (0.3, -0.2, 0.4)), (140.0, (3.5, -1.25, 0.75))):
        a = np.radians(yaw)
        Rcw = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        want, got = S.make_camera(W, H, yaw_deg=yaw, position=pos), IZ.camera(W, H, fx, fx, Rcw, pos)
        assert want.keys() == got.keys()
        for k in want:
            assert np.array_equal(want[k], got[k]) and np.asarray(want[k]).dtype == np.asarray(got[k]).dtype, (yaw, k)
    for pose in ("rpy", "zup"):
        want, got = PZ.camera(W, H, *PZ.POSES[pose]), IZ.camera(W, H, fx, fx, *PZ.POSES[pose])
        for k in want:
            assert np.array_equal(want[k], got[k]), (pose, k)
        w64, g64 = (PZ.camera(W, H, *PZ.POSES[pose], dtype=np.float64),
                    IZ.camera(W, H, fx, fx, *PZ.POSES[pose], dtype=np.float64))
        for k in ("viewmatrix", "campos"):
            assert np.array_equal(w64[k], g64[k]), (pose, k)
    sq = IZ.scene(300, W, H, 11, 3, fx, fx)              # ... and the scene over it is make_scene but for the background
    ms = S.make_scene(300, W, H, 11, sh_degree=3, bg=IZ.BG)
    for k in ms:
        if k == "means3D":                               # (fovx through atan and back, the aspect through two divisions)
            assert np.abs(sq[k] - ms[k]).max() <= 4 * U * np.abs(ms[k]).max()
        else:
            assert np.array_equal(sq[k], ms[k]) if ms[k] is not None else sq[k] is None, k


# ---------------------------------------------- the closed form ----------------------------------------------
# (W, H, fx, fy): W / 2fx and H / 2fy and their reciprocals are powers of two, so that tanfovx, tanfovy and the
# projection matrix's 1 / tanfov are exact in f32 and the closed form below, written from fx and fy, sees the very
# numbers the two restatements derive from the tangents.  fy / fx = 0.6 and 1.7.
CLOSED_CAMERAS = {"fy=0.6fx": (200, 60, 200.0, 120.0), "fy=1.7fx": (200, 170, 100.0, 170.0)}
# view-space (x, y, z), isotropic scale s; |x| / z against 1.3 tanfovx = 0.65 / 1.3, |y| / z against 1.3 tanfovy
CLOSED_SPLATS = {
    "on_axis": ((0.0, 0.0, 2.0), 0.0625),
    "off_axis": ((0.375, -0.21875, 1.5), 0.046875),
    "off_axis_far_corner": ((-0.5, 0.25, 1.25), 0.03125),
    "beyond_clamp_x": (("x", 1.5), 0.28125),
    "beyond_clamp_y": (("y", 1.5), 0.28125),
}


def _closed_case(cam, splat):
    W, H, fx, fy = CLOSED_CAMERAS[cam]
    pos, s = CLOSED_SPLATS[splat]
    tanx, tany = W / (2.0 * fx), H / (2.0 * fy)
    if isinstance(pos[0], str):        # 1.45 tanfov out on one axis, 0.25 tanfov on the other: clamped on that axis only
        axis, z = pos
        x, y = (1.45 * tanx * z, 0.25 * tany * z) if axis == "x" else (-0.25 * tanx * z, -1.45 * tany * z)
    else:
        x, y, z = pos
    x, y, z, s = (float(np.float32(v)) for v in (x, y, z, s))
    sc = dict(IZ.camera(W, H, fx, fy), means3D=np.array([[x, y, z]], np.float32), scales=np.full((1, 3), s, np.float32),
              rotations=np.array([[1.0, 0, 0, 0]], np.float32), opacities=np.array([[0.5]], np.float32),
              shs=np.zeros((1, 1, 3), np.float32), sh_degree=0, bg=np.zeros(3, np.float32), scale_modifier=1.0,
              colors_precomp=None, cov3D_precomp=None)
    assert sc["tanfovx"] == tanx and sc["tanfovy"] == tany and np.array_equal(sc["viewmatrix"], np.eye(4))
    assert sc["projmatrix"][0, 0] == 1.0 / tanx and sc["projmatrix"][1, 1] == 1.0 / tany
    return sc, (W, H, fx, fy, tanx, tany, x, y, z, s)


def _closed_form(W, H, fx, fy, tanx, tany, x, y, z, s):
    """f64, from fx and fy and nothing else of either restatement: cov2D = J s^2 J^T + 0.3 I with
    J = [[fx/z, 0, -fx x'/z^2], [0, fy/z, -fy y'/z^2]], (x', y') = (x, y) clamped to +-1.3 tanfov z (forward.cu:86-91);
    conic = cov2D^-1 as (A, B, C); radius = ceil(3 sqrt(lambda_max)); pixel centre ((ndc + 1) W - 1) / 2 with
    ndc = x / (tanfovx (z + 1e-7)) (the reference's p_w = 1 / (p_hom.w + 1e-7), forward.cu:232)."""
    xc = min(max(x / z, -1.3 * tanx), 1.3 * tanx) * z
    yc = min(max(y / z, -1.3 * tany), 1.3 * tany) * z
    J = np.array([[fx / z, 0.0, -fx * xc / z ** 2], [0.0, fy / z, -fy * yc / z ** 2]])
    cov = s * s * (J @ J.T) + 0.3 * np.eye(2)
    inv = np.linalg.inv(cov)
    lam = float(np.linalg.eigvalsh(cov).max())
    ndc = np.array([x / (tanx * (z + 1e-7)), y / (tany * (z + 1e-7))])
    pix = ((ndc + 1.0) * np.array([W, H]) - 1.0) * 0.5
    return dict(conic=np.array([inv[0, 0], inv[0, 1], inv[1, 1]]), cov=cov, r3=3.0 * math.sqrt(lam), ndc=ndc, pix=pix,
                clamped=(xc != x, yc != y))


@pytest.mark.parametrize("splat", list(CLOSED_SPLATS))
@pytest.mark.parametrize("cam", list(CLOSED_CAMERAS))
def test_closed_form_of_one_isotropic_gaussian(cam, splat):
    """One Gaussian with Sigma = s^2 I at view-space (x, y, z) under the identity view: conic, radius and pixel centre
    of the closed form (_closed_form) against ref64 to 1e-12 relative (ref64 computes no radius) and against the oracle
    within the f32 roundings of its operations.  With fy / fx = 0.6 or 1.7 a focal length read from the other axis
    moves A or C by a factor of up to 2.9 and B by 1.7.

    The oracle's roundings, in units of u = 2^-24, every intermediate relative to itself (inputs exact in f32; the
    identity view makes W m + t and T = W J exact):
      t' = (x / z clamped) * z: 2;  J00 = fx / z: 1;  J02 = -(fx t') / (z z): 2 + 3 = 5;  s^2: 1
      cov_xx = (J00 s^2) J00 + (J02 s^2) J02: each product chain adds 2 -> terms at 5 and 13, their sum 1: <= 14
      cov_xy = (J12 s^2) J02: 5 + 5 + 1 + 2 = 13;  a = cov_xx + 0.3f, c likewise: 0.3f is half an ulp off 0.3 and
      the sum rounds: <= 16 each
      det = a c - b b: products 16 + 16 + 1 = 33 and 13 + 13 + 1 = 27, the difference rounds once and is amplified by
      (a c + b b) / det <= 1.25 (asserted for each case): <= 1.25 * 33 + 1 < 43
      conic = c * (1 / det): 16 + 43 + 1 + 1 = 61 -> bound 64 u per element, relative to the element (B = 0 exactly
      on the axis).
    radius: 3 sqrt(mid + sqrt(mid^2 - det)) carries less than conic's 64 u; the case must not sit within that of an
    integer (asserted), then the two ceilings agree.  The reference floors mid^2 - det at 0.1 (forward.cu:263-264); the
    cases keep it above (asserted), so lambda_max is the true eigenvalue.
    pixel centre: ndc = (x / tanfov) * (1 / (z + 1e-7f)): 3, + 1: 1, * W: 1, - 1: 1, * 0.5 exact; each error at most
    u W (1 + |ndc|) / 2 in pixels, six of them: bound 4 u W (1 + |ndc|)."""
    sc, args = _closed_case(cam, splat)
    W, H = args[0], args[1]
    want = _closed_form(*args)
    assert want["clamped"] == {"beyond_clamp_x": (True, False), "beyond_clamp_y": (False, True)}.get(splat, (False, False))
    a, b, c = want["cov"][0, 0], want["cov"][0, 1], want["cov"][1, 1]
    assert (a * c + b * b) / (a * c - b * b) <= 1.25 and 0.25 * (a - c) ** 2 + b * b > 0.1
    assert (splat == "on_axis") == (b == 0.0)
    with torch.no_grad():
        _, g = R.per_gaussian(sc, [0])
    conic64, ndc64 = g["conic"][0].numpy(), g["ndc"][0].numpy()
    pix64 = ((ndc64 + 1.0) * np.array([W, H]) - 1.0) * 0.5
    assert np.abs(conic64 - want["conic"]).max() <= 1e-12 * np.abs(want["conic"]).max(), (conic64, want["conic"])
    assert (np.abs(conic64 - want["conic"]) <= 1e-12 * np.abs(want["conic"]) + 1e-300).all()
    assert (np.abs(pix64 - want["pix"]) <= 1e-12 * np.maximum(np.abs(want["pix"]), 1.0)).all(), (pix64, want["pix"])
    assert float(g["depth"][0]) == args[8]
    fr = O.forward(sc, keep_handle=False)
    radius = math.ceil(want["r3"])
    assert min(want["r3"] - (radius - 1), radius - want["r3"]) > 64 * U * want["r3"]
    assert fr.radii[0] == radius > 0, (fr.radii, want["r3"])
    got = fr.conic_opacity[0, :3].astype(np.float64)
    assert (np.abs(got - want["conic"]) <= 64 * U * np.abs(want["conic"])).all(), (got, want["conic"])
    tol = 4 * U * np.array([W, H]) * (1.0 + np.abs(want["ndc"]))
    assert (np.abs(fr.means2D[0].astype(np.float64) - want["pix"]) <= tol).all(), (fr.means2D, want["pix"])
    # what a swapped focal length would have given: far outside either bound
    swapped = _closed_form(W, H, args[3], args[2], *args[4:])
    assert np.abs(swapped["conic"] - want["conic"]).max() > 0.2 * np.abs(want["conic"]).max()


# ------------------------------------------ the oracle against ref64 ------------------------------------------
def _ratios(sc, seed):
    fr, r, g = _oracle_vs_f64(sc, seed)   # asserts the unchanged bars and the fragile cap of 0.5 %
    w = PZ.ratios_against_ref64(fr, r, g)
    print("oracle worst |d| / bar against f64: %.3f (%s)" % (max(w.values()), max(w, key=w.get)),
          {k: round(v, 3) for k, v in w.items()})
    return fr, r, g, w


@pytest.mark.parametrize("name", list(INTRINSICS))
def test_oracle_matches_f64_intrinsics(name):
    sc, seed = IZ.entry(name)
    fr, r, g, w = _ratios(sc, seed)
    assert max(w.values()) <= 0.5, w
    if name != "tiny":
        assert (fr.radii > 0).sum() > 0.85 * fr.P and np.abs(g["dL_dsh"][:, 1:]).max() > 0


@pytest.mark.parametrize("kind", IZ.PATHS)
def test_oracle_matches_f64_paths_intrinsics(kind):
    sc, seed = IZ.path_scene(kind)
    assert _focals_as_the_kernels_compute_them(sc)[0] != _focals_as_the_kernels_compute_them(sc)[1]
    fr, r, g, w = _ratios(sc, seed)
    assert max(w.values()) <= 0.5, w
    vis = fr.radii > 0
    if kind == "cov3D_precomp":   # (the same side conditions as tests/test_ref64.py: the path is really taken)
        assert np.abs(r["dL_dcov3D"]).max() > 0 and not g["dL_dscales"].any()
    elif kind == "jacobian_clamp":
        out = np.zeros(fr.P, bool)
        out[vis] = R.beyond_jacobian_clamp(sc, np.flatnonzero(vis)).numpy()
        assert out.sum() >= 10 and (np.abs(r["dL_dconic"][out]).max(axis=(1, 2)) > 0).sum() >= 10
    else:
        assert sc["scale_modifier"] == 0.7


def test_autograd_matches_finite_differences_with_two_focal_lengths():
    """gradcheck of the whole restated forward as in tests/test_ref64.py (same eps, atol, rtol, same preconditions),
    the five splats seen by `tiny`'s camera: fx = 20, fy = 31 at 33 x 17 under the zup pose (dense view matrix)."""
    W, H, fx, fy, pose, _ = INTRINSICS["tiny"]
    base = _gradcheck_scene()
    Rcw, T = PZ.POSES[pose]
    sc = dict(base, **IZ.camera(W, H, fx, fy, Rcw, T))
    sc["means3D"] = (base["means3D"].astype(np.float64) @ Rcw.T + T).astype(np.float32)
    assert np.abs(sc["viewmatrix"][:3, :3]).min() > 0
    _gradcheck_and_split_chain_rule(sc)


# ------------------------------------- the blind spot, recorded as a fact -------------------------------------
def _rejected(r, fragile, images, grads):
    """The groups of an f32 result that helpers.check_against_ref64 refuses."""
    bad = []
    for k, v in images.items():
        try:
            check_against_ref64(r, fragile, {k: v})
        except AssertionError:
            bad.append(k)
    for k in GRAD_NAMES:
        try:
            check_against_ref64(r, fragile, None, {k: grads[k]})
        except AssertionError:
            bad.append(k)
    return bad


def _truth(sc, seed):
    O.set_threads(1)
    fr = O.forward(sc)
    dcol, dacc = masked_upstream(sc["W"], sc["H"], seed, fr.fragile)
    return fr, dcol, dacc, R.render(sc, fr, dcol, dacc, slack=True)


@pytest.mark.parametrize("name", list(INTRINSICS))
def test_an_oracle_reading_focal_x_for_focal_y_is_rejected(name):
    """The oracle handed tangents for which its focal_y is its focal_x (intrinsics.with_fy_as_fx): in the backward
    alone (the right frame's own 2-D values, so only the conic -> covariance -> mean chain is wrong) ref64 refuses
    dL_dcov3D and what follows from it; in the forward as well, the images.  On every entry, ntu/4's 0.4 % included."""
    sc, seed = IZ.entry(name)
    fr, dcol, dacc, r = _truth(sc, seed)
    mut = IZ.with_fy_as_fx(sc)
    assert mut["tanfovy"] != sc["tanfovy"] and mut["tanfovx"] == sc["tanfovx"]
    g = O.backward(fr, mut, dcol, dacc)
    bad = _rejected(r, fr.fragile, {}, g)
    print(name, "backward with fy := fx, refused:", bad)
    assert {"dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"} <= set(bad), bad
    assert not {"dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors"} & set(bad)   # the blend reads no focal length
    fm = O.forward(mut)
    gm = O.backward(fm, mut, dcol, dacc)
    bad = _rejected(r, fr.fragile | fm.fragile, {k: getattr(fm, k) for k in IMAGES}, gm)
    print(name, "forward and backward with fy := fx, refused:", bad)
    assert "out_color" in bad and "out_acc" in bad and "dL_dconic" in bad, bad


def test_the_same_oracle_is_invisible_with_square_pixels():
    """... and on the suite's main scene, make_scene(1500, 200, 120, 13), the substitution changes no bit of any
    image or gradient: the tangent it derives is the scene's own."""
    seed = 13
    sc = S.make_scene(1500, 200, 120, seed, sh_degree=3)
    kx, ky = _focals_as_the_kernels_compute_them(sc)
    assert kx == ky
    mut = IZ.with_fy_as_fx(sc)
    fr, dcol, dacc, r = _truth(sc, seed)
    fm = O.forward(mut)
    for k in IMAGES + ("radii", "means2D", "conic_opacity", "point_list", "ranges", "n_contrib"):
        assert np.array_equal(getattr(fr, k), getattr(fm, k)), k
    g, gm = O.backward(fr, sc, dcol, dacc), O.backward(fm, mut, dcol, dacc)
    for k in GRAD_NAMES:
        assert np.array_equal(g[k], gm[k]), k
    assert not _rejected(r, fr.fragile, {k: getattr(fm, k) for k in IMAGES}, gm)
