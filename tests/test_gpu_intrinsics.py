"""GPU tests: the HIP path under cameras whose focal lengths differ (tests/intrinsics.py).

Every other camera of the suite has square pixels: focal_x = W / (2 tanfovx) and focal_y = H / (2 tanfovy) are the same
float there (one ulp apart at 70 x 50), and a kernel that reads one for the other -- ewa_project's J11 / J12, the
hx / hy of the per-Gaussian backward, make_params -- is bit-identical to the right one.  Here the checks of
tests/test_gpu_ref64.py (against f64) and tests/test_gpu_parity.py (against the oracle, exact stages bit for bit) on
every entry of intrinsics.INTRINSICS, the reference's own NTU calibration at a quarter of its size among them; the
product's forward variants and per-Gaussian backward over several blocks; the depth-gradient backward; a near/far
frame; render_utils.Camera, the autograd surface and the LibTorch surface; mark_visible."""
import functools
import math

import numpy as np
import pytest
import torch

import depth_ref as DR
import gs_livm_amd as G
import intrinsics as IZ
import poses as PZ
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, check_near_far_against_one_chain, grad_close, hip_backward, hip_forward, to_dev
from intrinsics import INTRINSICS
from oracle import oracle as O
from test_gpu_depth_grad import _backward as depth_backward
from test_gpu_depth_grad import _check_f64 as depth_check_f64
from test_gpu_depth_grad import _np
from test_gpu_parity import MODES, _full_check
from test_gpu_ref64 import _hip_vs_f64

pytestmark = pytest.mark.gpu


# ------------------------------------------------ against f64 ------------------------------------------------
@pytest.mark.parametrize("name", list(INTRINSICS))
def test_hip_matches_f64_intrinsics(name, gpu_device):
    """Both binning modes, debug and product forwards and backwards against one f64 evaluation, on scenes where the
    oracle alone stays at <= 0.5 of every bar (tests/test_intrinsics.py)."""
    sc, seed = IZ.entry(name)
    _hip_vs_f64(sc, seed, gpu_device)


@pytest.mark.parametrize("kind", IZ.PATHS)
def test_hip_matches_f64_paths_intrinsics(kind, gpu_device):
    sc, seed = IZ.path_scene(kind)
    _hip_vs_f64(sc, seed, gpu_device)


# --------------------------------------------- against the oracle ---------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ntu/4", "wide_y", "tall_y"])
def test_parity_intrinsics(name, mode, gpu_device):
    """test_gpu_parity's full check: radii, means2D, depths, conics, cov3D, keys, lists, ranges and n_contrib bit for
    bit, images to 1e-4, gradients to grad_close."""
    sc, seed = IZ.entry(name)
    fr, got = _full_check(sc, gpu_device, seed=seed, mode=mode)
    assert (fr.radii > 0).sum() > 1300 and np.abs(got["dL_dsh"][:, 1:]).max() > 0


@pytest.mark.parametrize("mode", MODES)
def test_parity_intrinsics_jacobian_clamp(mode, gpu_device):
    """Splats centred beyond 1.3 tanfov on one axis each, the two limits 1.3 tanfovx and 1.3 tanfovy apart by more
    than the aspect ratio: the clamped Jacobian's conics and radii bit for bit (the table's own scenes keep their
    splats within 1.1 tanfov and never clamp)."""
    sc, seed = IZ.path_scene("jacobian_clamp")
    fr, got = _full_check(sc, gpu_device, seed=seed, mode=mode)
    vis = np.flatnonzero(fr.radii > 0)
    out = R.beyond_jacobian_clamp(sc, vis).numpy()
    assert out.sum() >= 10 and (np.abs(got["dL_dconic"][vis[out]]).reshape(int(out.sum()), -1).max(1) > 0).sum() >= 10


def test_parity_intrinsics_precomputed_cov3d(gpu_device):
    sc, seed = IZ.path_scene("cov3D_precomp")
    fr, got = _full_check(sc, gpu_device, seed=seed)
    assert np.abs(got["dL_dcov3D"]).max() > 0 and not got["dL_dscales"].any() and not got["dL_drotations"].any()


# ---------------------------------------------- product variants ----------------------------------------------
@pytest.mark.parametrize("D", [1, 3])
def test_product_variants_intrinsics(D, gpu_device):
    """70 001 Gaussians at 320 x 200 (274 blocks, the last one partial), fx = 180, fy = 290, under the rpy pose: the
    non-debug forward's compile-time k_preprocess variants at SH degree 1 and 3 are bit-identical to the debug forward
    (images, radii, instance count), and the product's per-Gaussian backward (SH-staged at degree 3) equals ref64's
    per-Gaussian VJP fed with the HIP's own 2-D gradients, as test_product_variants_posed does with square pixels."""
    P, W, H, seed = 70_001, 320, 200, 31 + D
    sc = IZ.scene(P, W, H, seed, D, 180.0, 290.0, "rpy")
    t, dbg = hip_forward(sc, gpu_device, debug=True)
    for k in range(2):                                             # synchronous, then speculative
        t, prod = hip_forward(sc, gpu_device, debug=False)
        assert int(dbg[0]) == int(prod[0]) > 0
        for i in (1, 2, 3, 4):
            assert torch.equal(dbg[i], prod[i]), (k, i)
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    got = hip_backward(sc, t, prod, dcol, dacc, gpu_device, debug=False)
    radii = prod[4].cpu().numpy()
    two_d = np.concatenate([np.abs(got[k]).reshape(P, -1) for k in
                            ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors")], 1).max(1) > 0
    assert not two_d[radii <= 0].any()
    cand = np.flatnonzero(two_d)
    assert cand.size >= 1000
    idx = np.sort(np.random.default_rng(seed).choice(cand, size=min(4096, cand.size), replace=False))
    v = G.state_views(prod[5], prod[6], prod[7], P, prod[0], W, H)
    cl = v["clamped"].cpu().numpy()
    clamped = np.stack([(cl >> k) & 1 for k in range(3)], 1).astype(bool)
    g3 = R.gaussian_vjp(sc, idx, clamped, R.upstream_from_reference_arrays(got, idx))
    ref = {"dL_dmeans3D": g3["means3D"].numpy(), "dL_dcov3D": g3["cov6"].numpy(), "dL_dsh": g3["shs"].numpy(),
           "dL_dscales": g3["scales"].numpy(), "dL_drotations": g3["rotations"].numpy()}
    for k, want in ref.items():
        grad_close(got[k][idx], want, k)
    assert (np.abs(got["dL_dmeans3D"][idx]).max(1) > 0).all()


# ------------------------------------------- depth-gradient backward -------------------------------------------
@functools.lru_cache(maxsize=None)
def _depth_reference(name, mix):
    sc, seed = IZ.entry(name)
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc)
    up = DR.upstream(sc, fr, seed, mix)
    return sc, fr, up, DR.render64(sc, fr, *up, slack=True)


@pytest.mark.parametrize("mix", ["all", "depth_only"])
@pytest.mark.parametrize("name", ["wide_y", "tall_y"])
def test_depth_backward_matches_f64_intrinsics(name, mix, gpu_device):
    """gsr_backward_depth's ten outputs against depth_ref.render64 at the bound of tests/test_gpu_depth_grad.py, both
    binning modes, debug and product passes."""
    sc, fr, up, r = _depth_reference(name, mix)
    worst = {}
    for ref_rects in (True, False):
        for debug in (True, False):
            t, fwd = hip_forward(sc, gpu_device, debug=debug, ref_rects=ref_rects)
            got = _np(depth_backward(sc, t, fwd, up, gpu_device, debug=debug))
            for k, v in depth_check_f64(got, r).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(name, mix, "worst |d| / bar:", {k: round(v, 3) for k, v in worst.items()})
    assert np.abs(r["dL_ddepths"]).max() > 0 and np.abs(got["dL_ddepths"]).max() > 0
    assert np.abs(got["dL_dcov3D"]).max() > 0 and np.abs(got["dL_dmeans3D"]).max() > 0


# -------------------------------------------------- near/far --------------------------------------------------
def test_near_far_intrinsics(gpu_device):
    """A stack of opaque screen-filling splats in front of a camera with wide_y's focal lengths (scaled to
    320 x 208), binned near/far with a small near budget: bit-identical to the one-chain frame (images, n_contrib,
    every gradient)."""
    W0, H0, fx, fy, _, _ = INTRINSICS["wide_y"]
    W, H = 320, 208
    sc = IZ.scene(30_000, W, H, 23, 0, fx * W / W0, fy * W / W0)
    sc["means3D"][:64, :2] = 0.0
    sc["means3D"][:64, 2] = np.linspace(0.5, 0.9, 64, dtype=np.float32)
    sc["scales"][:64] = 0.29
    sc["opacities"][:64] = 0.98
    try:
        for near_entries in (8, 200):
            st = check_near_far_against_one_chain(sc, gpu_device, near_entries)
            assert 0 < st["near"] and st["near"] + st["far"] <= st["one"]
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


# ---------------------------------------- render_utils.Camera and render ----------------------------------------
def test_camera_class_intrinsics(gpu_device):
    """G.Camera(R, T, fovx, fovy, ...) with the two fields of view from tall_y's fx and fy: its matrices and the
    camera centre equal an f64 evaluation of the same formulas up to f32 rounding (the bound of
    test_camera_class_posed); the projection's two diagonal entries are 2 fx / W and 2 fy / H; render() through it
    is the direct operator call with the camera's tensors, bit for bit, and the oracle's frame of the same tensors."""
    W, H, fx, fy, pose, _ = INTRINSICS["tall_y"]
    Rcw, T = PZ.POSES[pose]
    D = 2
    fovx, fovy = IZ.focal2fov(fx, W), IZ.focal2fov(fy, H)
    cam = G.Camera(Rcw, T, fovx, fovy, W, H, device=gpu_device)
    want = IZ.camera(W, H, fx, fy, Rcw, T, dtype=np.float64)
    proj64 = S.projection_matrix(S.ZNEAR, S.ZFAR, fovx, fovy).astype(np.float64).T
    mag = 1.0 + float(np.abs(T).sum())
    eps = 16.0 * 2.0 ** -24
    for got, ref, bound in ((cam.Get_world_view_transform(), want["viewmatrix"], eps * mag),
                            (cam.Get_projection_matrix(), proj64, 0.0),
                            (cam.Get_full_proj_transform(), want["projmatrix"], eps * mag * np.abs(proj64).max()),
                            (cam.Get_camera_center(), want["campos"], eps * mag)):
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert np.abs(got.cpu().numpy().astype(np.float64) - ref).max() <= bound
    pm = cam.Get_projection_matrix().cpu().numpy().astype(np.float64)
    assert pm[0, 0] == pytest.approx(2.0 * fx / W, rel=2.0 ** -22)
    assert pm[1, 1] == pytest.approx(2.0 * fy / H, rel=2.0 ** -22)
    f32 = IZ.camera(W, H, fx, fy, Rcw, T)
    assert math.tan(cam.Get_FoVx() * 0.5) == pytest.approx(f32["tanfovx"], rel=1e-7)
    assert math.tan(cam.Get_FoVy() * 0.5) == pytest.approx(f32["tanfovy"], rel=1e-7)
    g = IZ.scene(1500, W, H, 31, D, fx, fy, pose)
    raw = dict(xyz=g["means3D"], f_dc=g["shs"][:, :1], f_rest=g["shs"][:, 1:], scaling=np.log(g["scales"]),
               rotation=g["rotations"] * 1.7, opacity=np.log(g["opacities"] / (1 - g["opacities"])))
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(gpu_device) for k, v in raw.items()}
    model = G.GaussianParameters(t["xyz"], t["f_dc"], t["f_rest"], t["scaling"], t["rotation"], t["opacity"])
    bg = torch.tensor(IZ.BG)
    color, depth, acc = G.render(cam, model, bg, 1.1)
    st = G.GaussianRasterizationSettings(H, W, math.tan(fovx * 0.5), math.tan(fovy * 0.5), bg.to(gpu_device), 1.1,
                                         cam.Get_world_view_transform(), cam.Get_full_proj_transform(), D,
                                         cam.Get_camera_center(), False)
    with torch.no_grad():
        xyz, op, sc, rot, shs = model.activated()
        c2, r2, d2, a2 = G.GaussianRasterizer(st)(xyz, torch.zeros_like(xyz), op, shs=shs, scales=sc, rotations=rot)
    assert torch.equal(color, c2) and torch.equal(depth, d2) and torch.equal(acc, a2)
    assert int((r2 > 0).sum()) > 1300 and float(acc.detach().max()) > 0.5     # the camera does see the scene
    sc_h = dict(g, scale_modifier=1.1, bg=bg.numpy(), scales=sc.cpu().numpy(), rotations=rot.cpu().numpy(),
                opacities=op.cpu().numpy(), shs=shs.cpu().numpy(),
                tanfovx=math.tan(fovx * 0.5), tanfovy=math.tan(fovy * 0.5),
                viewmatrix=cam.Get_world_view_transform().cpu().numpy(),
                projmatrix=cam.Get_full_proj_transform().cpu().numpy(), campos=cam.Get_camera_center().cpu().numpy())
    fr = O.forward(sc_h, keep_handle=False)
    ok = fr.fragile == 0
    assert np.array_equal(r2.cpu().numpy(), fr.radii)
    assert np.abs(color.detach().cpu().numpy() - fr.out_color).max(0)[ok].max() <= 1e-4


def test_autograd_surface_intrinsics(gpu_device):
    """tall_y through GaussianRasterizer and loss.backward(): the leaves receive hip_backward's gradients, finite and
    non-zero."""
    dev = gpu_device
    sc, seed = IZ.entry("tall_y")
    W, H = sc["W"], sc["H"]
    t, fwd = hip_forward(sc, dev, debug=False)
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    want = hip_backward(sc, t, fwd, dcol, dacc, dev, debug=False)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    st = G.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], t["bg"], 1.0, t["viewmatrix"],
                                         t["projmatrix"], 3, t["campos"], False)
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, depth, acc = G.GaussianRasterizer(st)(leaves["means3D"], means2D, leaves["opacities"],
                                                        shs=leaves["shs"], scales=leaves["scales"],
                                                        rotations=leaves["rotations"])
    assert torch.equal(color, fwd[1]) and torch.equal(radii, fwd[4]) and torch.equal(acc, fwd[3])
    ((color * torch.from_numpy(dcol).to(dev)).sum() + (acc * torch.from_numpy(dacc).to(dev)).sum()
     + 5.0 * depth.sum()).backward()
    for leaf, k in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh")):
        got = leaves[leaf].grad.cpu().numpy()
        assert np.isfinite(got).all() and np.abs(want[k]).max() > 0, k
        assert np.array_equal(got, want[k].reshape(leaves[leaf].shape)), k
    assert np.array_equal(means2D.grad.cpu().numpy(), want["dL_dmeans2D"])


def test_cpp_libtorch_surface_intrinsics(gpu_device):
    """The C++/LibTorch binding on wide_y: RasterizeGaussiansCUDA / ...BackwardCUDA are bit-equal to the C ABI route
    (each hands its two tangents through in its own order of arguments), and so is the GaussianRasterizer module
    through loss.backward()."""
    dev = gpu_device
    T = G.torch_ops()
    sc, seed = IZ.entry("wide_y")
    W, H, D = sc["W"], sc["H"], sc["sh_degree"]
    t, fwd = hip_forward(sc, dev)
    e = torch.empty(0, device=dev)
    out = T.RasterizeGaussiansCUDA(t["bg"], t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e,
                                   t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], H, W, t["shs"],
                                   D, t["campos"], False, False)
    assert T.last_num_rendered() == fwd[0] and out[0] >= fwd[0]
    for a, b in zip(out[1:5], fwd[1:5]):
        assert torch.equal(a, b)
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    dc, da = torch.from_numpy(dcol).to(dev), torch.from_numpy(dacc).to(dev)
    gb = T.RasterizeGaussiansBackwardCUDA(t["bg"], t["means3D"], out[4], e, t["scales"], t["rotations"], 1.0, e,
                                          t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], dc, da,
                                          t["shs"], D, t["campos"], out[5], out[0], out[6], out[7], False)
    ref = hip_backward(sc, t, fwd, dcol, dacc, dev)
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations")
    for n, g in zip(names, gb):
        assert np.abs(ref[n]).max() > 0 and np.array_equal(g.cpu().numpy(), ref[n]), n
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    st = T.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], t["bg"], 1.0, t["viewmatrix"],
                                         t["projmatrix"], D, t["campos"], False)
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, depth, acc = T.GaussianRasterizer(st).forward(leaves["means3D"], means2D, leaves["opacities"],
                                                                shs=leaves["shs"], scales=leaves["scales"],
                                                                rotations=leaves["rotations"])
    assert torch.equal(color, fwd[1]) and torch.equal(radii, fwd[4])
    ((color * dc).sum() + (acc * da).sum() + depth.sum()).backward()
    for leaf, n in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh")):
        assert np.array_equal(leaves[leaf].grad.cpu().numpy(), ref[n].reshape(leaves[leaf].shape)), n
    assert np.array_equal(means2D.grad.cpu().numpy(), ref["dL_dmeans2D"])


# ------------------------------------------------ mark_visible ------------------------------------------------
@pytest.mark.parametrize("name", ["wide_y", "tall_y"])
def test_mark_visible_intrinsics(name, gpu_device):
    """mark_visible depends on the view matrix only (the near cull t.z > 0.2): under either camera it equals the
    oracle's, and the projection matrix it is handed changes nothing -- splats far outside the narrow side of the
    frustum stay visible.  Guards against a frustum test written with one tangent."""
    W, H, fx, fy, pose, _ = INTRINSICS[name]
    # laid out over a frustum three times as wide as the camera's on both axes: most splats are outside the image
    sc = IZ.scene(3000, W, H, 17, 0, fx / 3.0, fy / 3.0, pose)
    sc.update(IZ.camera(W, H, fx, fy, *((np.eye(3), np.zeros(3)) if pose is None else PZ.POSES[pose])))
    t = to_dev(sc, gpu_device)
    want = O.mark_visible(sc["means3D"], sc["viewmatrix"])
    assert 2800 < want.sum() < 3000                                 # the 2 % behind the camera stay invisible
    tv = sc["means3D"].astype(np.float64) @ sc["viewmatrix"][:3, :3] + sc["viewmatrix"][3, :3]
    outside = (np.abs(tv[:, 0]) > sc["tanfovx"] * tv[:, 2]) | (np.abs(tv[:, 1]) > sc["tanfovy"] * tv[:, 2])
    assert (want & outside).sum() > 1500
    got = G.mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"]).cpu().numpy()
    assert np.array_equal(got, want)
    other = IZ.camera(W, H, fy, fx, *((np.eye(3), np.zeros(3)) if pose is None else PZ.POSES[pose]))
    got2 = G.mark_visible(t["means3D"], t["viewmatrix"], torch.from_numpy(other["projmatrix"]).to(gpu_device))
    assert np.array_equal(got2.cpu().numpy(), want)
