"""CPU tests of tests/lidar_ref.py (the restatement of the LiDAR depth supervision the GPU tests hold csrc/lidar.hip to)
and of loss.raster_K / loss.world_to_camera: the float64 loop equals the float64 Torch ops exactly, gradcheck, closed
forms (the exact-arithmetic scenes bit for bit; the pixel convention against the oracle's rasterizer), and -- what
licenses the 1 % caps of tests/test_gpu_lidar.py -- the fragile shares and the float32 restatement on every GPU-test
input."""
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import intrinsics as I
import lidar_ref as L
import poses as PZ
from oracle import oracle as O

F64 = torch.float64


@pytest.mark.parametrize("case", L.CASE_NAMES + L.EXACT_NAMES)
def test_loop_equals_float64_ops_exactly(case):
    x = L.inputs(case)
    img, kept, hit, _ = L.image64(*L._image_args(x))
    ops, kept_o, hit_o = L.image_ops(*L._image_args(x), dtype=F64)
    assert (kept, hit) == (kept_o, hit_o)
    assert np.array_equal(ops.numpy(), img)
    assert hit == int((img > 0).sum()) and kept >= hit


def test_gradcheck_smooth_case():
    """away from the kinks: every |e| >= 0.05 m, every A at least 0.05 from acc_min"""
    rng = np.random.default_rng(3)
    H, W = 6, 7
    zl = rng.uniform(2.0, 8.0, (H, W))
    zl[1, 2] = zl[4, 5] = 0.0                                            # holes
    A = np.where(rng.uniform(0, 1, (H, W)) < 0.3, rng.uniform(0.2, 0.45, (H, W)), rng.uniform(0.55, 1.0, (H, W)))
    D = A * (np.where(zl > 0, zl, 5.0) + rng.uniform(0.05, 0.4, (H, W)) * (rng.integers(0, 2, (H, W)) * 2 - 1))
    t = lambda a: torch.as_tensor(a, dtype=F64)  # noqa: E731
    d, a = t(D).clone().requires_grad_(True), t(A).clone().requires_grad_(True)
    fn = lambda d, a: L.loss_forward_ops(d, a, t(zl), 0.5, 0.7)[0]  # noqa: E731
    assert torch.autograd.gradcheck(fn, (d, a), eps=1e-6, atol=1e-9, rtol=1e-6)
    # and the closed form of include/gsraster.h is that gradient
    r = L.loss_ops(D, A, zl, 0.5, 0.7)
    sup = (zl > 0) & (A >= 0.5)
    n = int(sup.sum())
    assert 0 < n < H * W and abs(float(r["share"]) - n / (H * W)) <= 1e-15
    e = np.where(sup, D / A - zl, 0.0)
    c = 0.7 / n
    assert abs(float(r["mean"]) - np.abs(e).sum() / n) <= 1e-14 and abs(float(r["loss"]) - 0.7 * np.abs(e).sum() / n) <= 1e-14
    assert np.abs(r["grad_depth"].numpy() - np.where(sup, c * np.sign(e) / A, 0.0)).max() <= 1e-15
    assert np.abs(r["grad_acc"].numpy() - np.where(sup, -c * np.sign(e) * D / A ** 2, 0.0)).max() <= 1e-14


def test_unsupervised_frame_is_all_zero():
    r = L.loss_ops(np.ones((3, 4)), np.full((3, 4), 0.4), np.full((3, 4), 2.0))
    assert float(r["loss"]) == 0 and float(r["mean"]) == 0 and float(r["share"]) == 0
    assert not r["grad_depth"].any() and not r["grad_acc"].any()


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_fragile_shares_and_float32_restatement_on_gpu_inputs(case):
    """The fragile sets stay at or below 1 % of the points and of the pixels on every input of
    tests/test_gpu_lidar.py, and the float32 restatement stays inside every bar on what is compared."""
    x, ref = L.inputs(case), L.reference(case)
    shares = L.fragile_shares(ref, x)
    im, lo = ref["image"], ref["loss"]
    ri = L.image_ratios(im["f32"], im["kept32"], im["hit32"], ref)
    rl = L.loss_ratios({k: lo["f32"][k].to(F64) for k in lo["f32"]}, ref)
    print(case, "fragile points %.4f image pixels %.4f loss pixels %.4f" % shares, "float32 |d| / bar:",
          {k: round(v, 3) for k, v in {**ri, **rl}.items()})
    assert max(shares) <= 0.01, shares
    assert max(ri.values()) <= 1.0 and max(rl.values()) <= 1.0, (ri, rl)


def test_inputs_exercise_what_they_claim():
    seen = dict(behind=0, several=0, nan=0, inf=0, low_acc=0, at_acc_min=0, holes=0, beyond_max=0, outside=0, zero_e=0)
    for case in L.CASE_NAMES:
        x, ref = L.inputs(case), L.reference(case)
        e = L.project64(x["points"], x["T_cw"], x["K"])
        seen["behind"] += int((e["z"][e["finite"]] < 0).sum())
        seen["beyond_max"] += int((e["z"][e["finite"]] > x["max_depth"]).sum())
        seen["outside"] += int((e["finite"] & (e["z"] > 1) & (e["X"] < -0.5)).sum())
        seen["several"] += int(ref["image"]["kept"] - ref["image"]["hit"])
        seen["nan"] += int(np.isnan(x["points"]).sum())
        seen["inf"] += int(np.isinf(x["points"]).sum())
        seen["low_acc"] += int(((x["acc"] < x["acc_min"]) & (x["lidar"] > 0)).sum())
        seen["at_acc_min"] += int(((x["acc"] == np.float32(x["acc_min"])) & (x["lidar"] > 0)).sum())
        seen["holes"] += int((x["lidar"] == 0).sum())
        seen["zero_e"] += int((ref["loss"]["truth"]["grad_depth"][torch.as_tensor((x["lidar"] > 0) & (x["acc"] == 1))] == 0).sum())
        if x["n"] >= 8:
            assert np.isnan(x["points"]).sum() == 1 and np.isinf(x["points"]).sum() == 1
        if x["n"] > 0:
            assert 0 < ref["loss"]["n_sup"] <= ref["image"]["hit"]
    assert all(v > 0 for v in seen.values()), seen
    assert L.reference("3x5_n0")["loss"]["n_sup"] == 0                      # the unsupervised frame
    R = L.pose("rpy")[:, :3]
    assert all(abs(v) > 1e-3 for v in R.reshape(-1)) and np.abs(R - R.T).max() > 0.1
    assert np.abs(L.pose("yaw")[:, :3] - L.pose("yaw")[:, :3].T).max() > 0.1
    for case in L.CASE_NAMES[1:]:
        K = L.inputs(case)["K"]
        assert K[0, 0] != K[1, 1] and K[0, 2] != (L.inputs(case)["W"] - 1) / 2


@pytest.mark.parametrize("case", L.EXACT_NAMES)
def test_exact_scenes_are_known_bit_for_bit(case):
    """Identity pose, power-of-two focal lengths, dyadic coordinates: X, Y and z carry no rounding in any evaluation
    order, so float32 and float64 agree exactly and the special points land where the contract says."""
    x, ref = L.inputs(case), L.reference(case)
    H, W = x["H"], x["W"]
    img = ref["image"]
    ops32, kept32, hit32 = L.image_ops(*L._image_args(x), dtype=torch.float32)
    assert np.array_equal(ops32.numpy().astype(np.float64), img) and (kept32, hit32) == (ref["kept"], ref["hit"])
    e = ref["proj"]
    assert np.array_equal(e["X"] * 4, np.round(e["X"] * 4)) and np.array_equal(e["Y"] * 4, np.round(e["Y"] * 4))
    # the last two rows hold the special points only
    want = np.zeros((2, W))
    want[0, 0] = 2.0                  # X = -0.5: inside, pixel 0 (and X = W - 0.5 is outside: [H-2, W-1] stays 0)
    want[1, 2] = L.EXACT_MAX          # z == max_depth is kept; z == min_depth [H-1, 0] and 2 max_depth [H-1, 4] are not
    assert np.array_equal(img[H - 2:], want)
    assert float(img.max()) == L.EXACT_MAX and float(img[img > 0].min()) > L.EXACT_MIN
    assert ref["kept"] > ref["hit"] > 2
    # Y = -0.5 lands in row 0, X + 0.5 == W does not land
    top = e["finite"] & (e["Y"] == -0.5) & (e["X"] >= -0.5) & (e["X"] < W - 0.5) & (e["z"] > L.EXACT_MIN) & (e["z"] <= L.EXACT_MAX)
    assert top.any()
    for i in np.nonzero(top)[0]:
        assert 0 < img[0, math.floor(e["X"][i] + 0.5)] <= e["z"][i]


def test_raster_K_and_world_to_camera_against_the_oracle():
    """One small isotropic Gaussian at a posed point p: the oracle rasterizer's brightest pixel is the one pixel where
    the LiDAR image of [p] is non-zero, and that value is the oracle's depth of the Gaussian (rpy pose, fx != fy)."""
    W, H, fx, fy = 57, 41, 52.0, 71.0
    R_cw, T = PZ.POSES["rpy"]
    fovx, fovy = I.focal2fov(fx, W), I.focal2fov(fy, H)
    K = G.raster_K(W, H, fovx, fovy)
    assert K.dtype == F64 and tuple(K.shape) == (3, 3)
    assert abs(float(K[0, 0]) - fx) <= 1e-9 and abs(float(K[1, 1]) - fy) <= 1e-9
    assert float(K[0, 2]) == (W - 1) / 2 and float(K[1, 2]) == (H - 1) / 2
    cam = G.Camera(R_cw, T, fovx, fovy, W, H, device="cpu")
    T_cw = G.world_to_camera(cam)
    assert T_cw.dtype == torch.float32 and tuple(T_cw.shape) == (3, 4)
    assert np.abs(T_cw.numpy()[:, :3] - R_cw.T).max() <= 1e-6 and np.abs(T_cw.numpy()[:, 3] + R_cw.T @ T).max() <= 1e-5
    assert np.abs(T_cw.numpy()[:, :3] - R_cw).max() > 0.1          # the transposed matrix is another one
    for (u, v, z) in ((40.2, 9.9, 3.7), (3.1, 30.8, 6.2)):
        p_cam = np.array([(u - float(K[0, 2])) / fx * z, (v - float(K[1, 2])) / fy * z, z])
        p = (R_cw @ p_cam + T).astype(np.float32)
        sc = I.scene(1, W, H, 1, 0, fx, fy, pose="rpy")
        sc["means3D"] = p[None].copy()
        sc["scales"] = np.full((1, 3), 0.01, np.float32)
        sc["rotations"] = np.array([[1, 0, 0, 0]], np.float32)
        sc["opacities"] = np.full((1, 1), 0.9, np.float32)
        fr = O.forward(sc, keep_handle=False)
        acc = np.asarray(fr.out_acc, np.float64).reshape(H, W)
        iy, ix = np.unravel_index(int(np.argmax(acc)), acc.shape)
        assert acc[iy, ix] > 0.5
        img, kept, hit, _ = L.image64(p[None], T_cw.numpy(), K.numpy().astype(np.float32), H, W)
        assert (kept, hit) == (1, 1)
        assert (int(iy), int(ix)) == (round(v), round(u)) and img[iy, ix] > 0
        assert abs(img[iy, ix] - float(fr.depths[0])) <= 1e-6 * float(fr.depths[0])
        # with fx read for fy, or R transposed, the point lands elsewhere (or nowhere)
        Kbad = K.numpy().copy()
        Kbad[1, 1] = Kbad[0, 0]
        assert L.image64(p[None], T_cw.numpy(), Kbad, H, W)[0][iy, ix] == 0
        Tbad = T_cw.numpy().copy()
        Tbad[:, :3] = Tbad[:, :3].T
        assert L.image64(p[None], Tbad, K.numpy(), H, W)[0][iy, ix] == 0
