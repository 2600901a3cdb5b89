"""GPU tests: the HIP path under rolled, pitched and translated cameras (tests/poses.py).

Every other camera of the suite is a yaw about +y: viewmatrix[1], [4], [6] and [9] are exactly 0 there, and a kernel
that reads the matrix transposed in those places -- k_preprocess and its SH variants, the per-Gaussian backward,
mark_visible, the EWA T = W J -- is bit-identical to the right one.  Here the same checks as tests/test_gpu_ref64.py
(against f64, every pose within poses.REACH) and tests/test_gpu_parity.py (against the oracle, exact stages bit for
bit, the `far` pose of hundreds of metres included), the product's forward variants and per-Gaussian backward over
several blocks, mark_visible, a near/far frame, render_utils.Camera and the autograd surface, all with dense view
matrices."""
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import poses as PZ
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import check_near_far_against_one_chain, grad_close, hip_backward, hip_forward, to_dev
from oracle import oracle as O
from poses import POSES, WITHIN_REACH, posed
from test_gpu_parity import MODES, _full_check
from test_gpu_ref64 import _hip_vs_f64
from test_poses import BIG, BIG_POSE, SCENES

pytestmark = pytest.mark.gpu
PATHS = ("cov3D_precomp", "jacobian_clamp", "sh_clamp", "scale_modifier")


def _scene(spec, pose):
    P, W, H, seed, D = spec
    return posed(S.make_scene(P, W, H, seed, sh_degree=D), *POSES[pose]), seed


# ------------------------------------------------ against f64 ------------------------------------------------
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("pose", WITHIN_REACH)
def test_hip_matches_f64_posed(pose, scene, gpu_device):
    """Both binning modes, debug and product forwards and backwards against one f64 evaluation, at poses where the
    oracle alone stays at <= 0.5 of every bar (tests/test_poses.py)."""
    sc, seed = _scene(SCENES[scene], pose)
    _hip_vs_f64(sc, seed, gpu_device)


def test_hip_matches_f64_posed_big(gpu_device):
    sc, seed = _scene(BIG, BIG_POSE)
    _hip_vs_f64(sc, seed, gpu_device)


@pytest.mark.parametrize("pose", ["rpy", "zup"])
@pytest.mark.parametrize("kind", PATHS)
def test_hip_matches_f64_paths_posed(kind, pose, gpu_device):
    sc, seed = PZ.posed_path_scene(kind, *POSES[pose])
    _hip_vs_f64(sc, seed, gpu_device)


# --------------------------------------------- against the oracle ---------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pose", list(POSES))
def test_parity_posed(pose, mode, gpu_device):
    """test_gpu_parity's full check on every pose: radii, means2D, depths, conics, cov3D, keys, lists, ranges and
    n_contrib bit for bit, images to 1e-4, gradients to grad_close.  At `far` the coordinates are hundreds of metres:
    the exact stages still equal the oracle's bit for bit (same association order, no contraction), which is where an
    accidental FMA in W m + t would show."""
    sc, seed = _scene(SCENES["P1500_D3"], pose)
    fr, got = _full_check(sc, gpu_device, seed=seed, mode=mode)
    assert (fr.radii > 0).sum() > 1300 and np.abs(got["dL_dsh"][:, 1:]).max() > 0


@pytest.mark.parametrize("pose", ["rpy", "zup", "far"])
def test_parity_posed_precomputed_cov3d(pose, gpu_device):
    """The world-frame covariance that only the view matrix turns into the camera frame."""
    sc, seed = PZ.posed_path_scene("cov3D_precomp", *POSES[pose])
    fr, got = _full_check(sc, gpu_device, seed=seed)
    assert np.abs(got["dL_dcov3D"]).max() > 0 and not got["dL_dscales"].any() and not got["dL_drotations"].any()


# ---------------------------------------------- product variants ----------------------------------------------
@pytest.mark.parametrize("pose", ["rpy", "zup"])
@pytest.mark.parametrize("D", [1, 3])
def test_product_variants_posed(D, pose, gpu_device):
    """70 001 Gaussians at 320 x 200 (274 blocks, the last one partial): the non-debug forward's compile-time
    k_preprocess variants at SH degree 1 and 3 are bit-identical to the debug forward (images, radii, instance count),
    and the product's per-Gaussian backward (SH-staged at degree 3) equals ref64's per-Gaussian VJP fed with the HIP's
    own 2-D gradients, as test_per_gaussian_stage_at_scale does at the origin."""
    P, W, H, seed = 70_001, 320, 200, 31 + D
    sc = posed(S.make_scene(P, W, H, seed, sh_degree=D), *POSES[pose])
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


# ------------------------------------------------ mark_visible ------------------------------------------------
@pytest.mark.parametrize("pose", list(POSES))
def test_mark_visible_posed(pose, gpu_device):
    sc = posed(S.make_scene(3000, 64, 48, 17), *POSES[pose])
    t = to_dev(sc, gpu_device)
    want = O.mark_visible(sc["means3D"], sc["viewmatrix"])
    assert 100 < want.sum() < 3000                                 # the 2 % behind the camera stay invisible
    assert np.array_equal(G.mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"]).cpu().numpy(), want)
    # the same world seen from the origin camera: nearly everything is on the wrong side now
    origin = S.make_camera(64, 48)
    want0 = O.mark_visible(sc["means3D"], origin["viewmatrix"])
    got0 = G.mark_visible(t["means3D"], torch.from_numpy(origin["viewmatrix"]).to(gpu_device),
                          torch.from_numpy(origin["projmatrix"]).to(gpu_device)).cpu().numpy()
    assert np.array_equal(got0, want0)


# -------------------------------------------------- near/far --------------------------------------------------
def test_near_far_posed(gpu_device):
    """A stack of opaque screen-filling splats in front of the zup camera, binned near/far with a small near budget:
    bit-identical to the one-chain frame (images, n_contrib, every gradient)."""
    sc = S.make_scene(30_000, 320, 208, 23, sh_degree=0)
    sc["means3D"][:64, :2] = 0.0
    sc["means3D"][:64, 2] = np.linspace(0.5, 0.9, 64, dtype=np.float32)
    sc["scales"][:64] = 0.29
    sc["opacities"][:64] = 0.98
    sc = posed(sc, *POSES["zup"])
    try:
        for near_entries in (8, 200):
            st = check_near_far_against_one_chain(sc, gpu_device, near_entries)
            assert 0 < st["near"] and st["near"] + st["far"] <= st["one"]
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


# ---------------------------------------- render_utils.Camera and render ----------------------------------------
@pytest.mark.parametrize("pose", list(POSES))
def test_camera_class_posed(pose, gpu_device):
    """G.Camera(R, T, ...): its three matrices and the camera centre equal an f64 evaluation of the same formulas up
    to f32 rounding (every entry is a sum of at most four products of an entry <= 1 + |T|_1 with a projection entry;
    16 roundings of that magnitude bound it with room, a transposed or mis-signed entry is off by O(0.1)); render()
    through it is the direct operator call with the camera's tensors, bit for bit."""
    Rcw, T = POSES[pose]
    W, H, D = 200, 120, 2
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    cam = G.Camera(Rcw, T, fovx, fovy, W, H, device=gpu_device)
    want = PZ.camera(W, H, Rcw, T, dtype=np.float64)
    proj64 = S.projection_matrix(S.ZNEAR, S.ZFAR, fovx, fovy).astype(np.float64).T
    mag = 1.0 + float(np.abs(T).sum())
    eps = 16.0 * 2.0 ** -24
    for got, ref, bound in ((cam.Get_world_view_transform(), want["viewmatrix"], eps * mag),
                            (cam.Get_projection_matrix(), proj64, 0.0),
                            (cam.Get_full_proj_transform(), want["projmatrix"], eps * mag * np.abs(proj64).max()),
                            (cam.Get_camera_center(), want["campos"], eps * mag)):
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert np.abs(got.cpu().numpy().astype(np.float64) - ref).max() <= bound
    # the helper's own f32 camera is the same camera
    f32 = PZ.camera(W, H, Rcw, T)
    assert np.abs(cam.Get_world_view_transform().cpu().numpy() - f32["viewmatrix"]).max() <= eps * mag
    assert math.tan(cam.Get_FoVx() * 0.5) == pytest.approx(f32["tanfovx"], rel=1e-7)
    g = posed(S.make_scene(1500, W, H, 31, sh_degree=D), Rcw, T)
    raw = dict(xyz=g["means3D"], f_dc=g["shs"][:, :1], f_rest=g["shs"][:, 1:], scaling=np.log(g["scales"]),
               rotation=g["rotations"] * 1.7, opacity=np.log(g["opacities"] / (1 - g["opacities"])))
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(gpu_device) for k, v in raw.items()}
    model = G.GaussianParameters(t["xyz"], t["f_dc"], t["f_rest"], t["scaling"], t["rotation"], t["opacity"])
    bg = torch.tensor([0.2, 0.5, 0.9])
    color, depth, acc = G.render(cam, model, bg, 1.1)
    st = G.GaussianRasterizationSettings(H, W, math.tan(fovx * 0.5), math.tan(fovy * 0.5), bg.to(gpu_device), 1.1,
                                         cam.Get_world_view_transform(), cam.Get_full_proj_transform(), D,
                                         cam.Get_camera_center(), False)
    with torch.no_grad():
        xyz, op, sc, rot, shs = model.activated()
        c2, r2, d2, a2 = G.GaussianRasterizer(st)(xyz, torch.zeros_like(xyz), op, shs=shs, scales=sc, rotations=rot)
    assert torch.equal(color, c2) and torch.equal(depth, d2) and torch.equal(acc, a2)
    assert int((r2 > 0).sum()) > 1300 and float(acc.detach().max()) > 0.5     # the camera does see the scene
    # ... and the frame is the oracle's of the same tensors, to the image bar off the oracle's fragile pixels
    sc_h = dict(g, scale_modifier=1.1, bg=bg.numpy(), scales=sc.cpu().numpy(), rotations=rot.cpu().numpy(),
                opacities=op.cpu().numpy(), shs=shs.cpu().numpy(),
                viewmatrix=cam.Get_world_view_transform().cpu().numpy(),
                projmatrix=cam.Get_full_proj_transform().cpu().numpy(), campos=cam.Get_camera_center().cpu().numpy())
    fr = O.forward(sc_h, keep_handle=False)
    ok = fr.fragile == 0
    assert np.abs(color.detach().cpu().numpy() - fr.out_color).max(0)[ok].max() <= 1e-4


# ----------------------------------------------- autograd surface -----------------------------------------------
def test_autograd_surface_posed(gpu_device):
    """One posed view through GaussianRasterizer and loss.backward(): the leaves receive hip_backward's gradients."""
    dev = gpu_device
    sc, seed = _scene(SCENES["P1500_D3"], "rpy")
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
        assert np.abs(want[k]).max() > 0
        assert np.array_equal(leaves[leaf].grad.cpu().numpy(), want[k].reshape(leaves[leaf].shape)), k
    assert np.array_equal(means2D.grad.cpu().numpy(), want["dL_dmeans2D"])
