"""GPU tests of the depth-normal consistency loss (csrc/normal.hip through gsr_normal_consistency_loss and
gs_livm_amd.normal_consistency_loss) on synthetic images, with no rasterizer in the way.

Reference: tests/normal_ref.py -- float64 Torch ops with autograd (held to closed forms and gradcheck by
tests/test_normal_ref.py).  Bars = 8 x the float32 yardstick's worst error over these very cases: out3 relative to the
value (B_OUT3 = 1.04e-6), the gradients relative to the image's largest |g64| (B_GRADS = 5.92e-5).  The supervised
count is exact."""
import functools
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import normal_ref as NR

pytestmark = pytest.mark.gpu
INF = float("inf")


def _gpu(D, A, N, cam, acc_min, normal_min, jump_rel, lam, dev, grads=(True, True), prefill=False):
    """numpy in, numpy out: (out3, dL/dD or None, dL/dA or None)"""
    d, a, n = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) for x in (D, A, N))
    out3, gd, ga = _capi.normal_consistency_loss(d, a, n, *cam, acc_min, normal_min, jump_rel, lam,
                                                 want_grad_depth=grads[0], want_grad_acc=grads[1])
    f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return f(out3), f(gd), f(ga)


def _count(out3, W, H):
    return int(round(float(out3[2]) * W * H))


@functools.lru_cache(maxsize=None)
def _reference(W, H, seed, jump):
    D, A, N, cam = NR.loss_case(W, H, seed)
    return (D, A, N, cam) + NR.loss_and_grads(D, A, N, cam, jump_rel=jump, **NR.CASE_KW)


# ---- against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jump", NR.JUMPS)
@pytest.mark.parametrize("W,H", NR.SHAPES)
def test_loss_and_gradients_equal_float64_at_the_bars(W, H, jump, gpu_device):
    kw = NR.CASE_KW
    for seed in NR.SEEDS:
        D, A, N, cam, out64, gd64, ga64, S, _ = _reference(W, H, seed, jump)
        out3, gd, ga = _gpu(D, A, N, cam, kw["acc_min"], kw["normal_min"], jump, kw["lam"], gpu_device)
        assert _count(out3, W, H) == S
        ro, rd, ra = NR.rel(out3, out64), NR.grad_ratio(gd, gd64), NR.grad_ratio(ga, ga64)
        print("%d x %d seed %d jump %s: S %d  out3 %.3e (bar %.3e)  dL/dD %.3e  dL/dA %.3e (bar %.3e)"
              % (W, H, seed, jump, S, ro, NR.B_OUT3, rd, ra, NR.B_GRADS))
        assert ro <= NR.B_OUT3 and rd <= NR.B_GRADS and ra <= NR.B_GRADS
        if S:
            assert np.abs(gd64).max() > 0
    assert W != 3 or _reference(W, H, 0, INF)[7] == 1    # 3 x 3: one candidate


@pytest.mark.parametrize("theta_deg", [0.0, 10.0, 75.0])
def test_a_tilted_plane_gives_one_minus_cos_theta(theta_deg, gpu_device):
    W, H = 37, 23
    theta = math.radians(theta_deg)
    D, A, N, cam, _ = NR.plane_case(W, H, theta=theta)
    out3, gd, ga = _gpu(D, A, N, cam, 0.5, 0.1, INF, 2.0, gpu_device)
    want = 1.0 - math.cos(theta)
    assert _count(out3, W, H) == (W - 2) * (H - 2)
    # against float64 on the same float32 images at the bar (relative to the value; at theta = 0 the value is a difference
    # of two numbers near 1, whose float32 error the bar is then relative to) ...
    ref = NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, INF, 2.0)[0]
    print("theta %g: mean rho %.9f  float64 %.9f  closed form %.9f" % (theta_deg, out3[1], ref[1], want))
    assert abs(float(out3[1]) - ref[1]) <= NR.B_OUT3 * max(ref[1], 1.0 if theta == 0.0 else 0.0)
    assert abs(float(out3[0]) - ref[0]) <= NR.B_OUT3 * max(ref[0], 2.0 if theta == 0.0 else 0.0)
    # ... and the closed form itself: rounding the plane's depths to float32 moves a and b by 2^-24 |X| / |a| ~ 1e-6
    # relative, rho by less than that (measured in float64: 1.6e-8)
    assert abs(float(out3[1]) - want) <= 1e-6
    if theta_deg == 10.0:    # the orientation of c: a x b for b x a would give 1 + cos(theta)
        assert float(out3[1]) < 0.1


def test_the_principal_point_is_the_centre_of_the_pixel_grid(gpu_device):
    # cx = W / 2 for (W - 1) / 2 tilts every ray: on this steep plane rho rises from rounding level to 1.0e-5 (float64)
    W, H = 37, 23
    D, A, N, cam, _ = NR.plane_case(W, H, normal=(0.6, -0.4, -1.0))
    good = _gpu(D, A, N, cam, 0.5, 0.1, INF, 1.0, gpu_device)[0]
    off = _gpu(D, A, N, (cam[0], cam[1], W / 2.0, cam[3]), 0.5, 0.1, INF, 1.0, gpu_device)[0]
    print("rho with cx = (W - 1) / 2: %.3e, with W / 2: %.3e" % (good[1], off[1]))
    assert abs(float(good[1])) <= NR.B_OUT3 and float(off[1]) > 5e-6


# ---- shapes without an interior, nothing supervised ----------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(2, 2), (1, 7), (7, 1)])
def test_images_without_an_interior_give_zero(W, H, gpu_device):
    D, A, N, cam = NR.loss_case(W, H)
    out3, gd, ga = _gpu(D, A, N, cam, 0.5, 0.1, INF, 1.0, gpu_device)
    assert not out3.view(np.int32).any() and not gd.view(np.int32).any() and not ga.view(np.int32).any()


def test_nothing_supervised_gives_zero_without_nan(gpu_device):
    D, A, N, cam = NR.loss_case(16, 17)
    for kw in (dict(acc_min=2.0), dict(normal_min=5.0), dict(jump_rel=0.0)):
        args = dict(acc_min=0.5, normal_min=0.1, jump_rel=INF)
        args.update(kw)
        out3, gd, ga = _gpu(D, A, N, cam, args["acc_min"], args["normal_min"], args["jump_rel"], 1.0, gpu_device)
        assert not out3.view(np.int32).any() and not gd.view(np.int32).any() and not ga.view(np.int32).any(), kw


# ---- gates, as exact counts -------------------------------------------------------------------------------------------------
def test_gates_remove_exactly_the_predicted_pixels(gpu_device):
    dev = gpu_device
    W, H = 16, 17
    D, A, N, cam = NR.loss_case(W, H)
    full = (W - 2) * (H - 2)
    assert _count(_gpu(D, A, N, cam, 0.5, 0.1, INF, 1.0, dev)[0], W, H) == full
    # one pixel below acc_min: itself and its four neighbours
    A1, D1 = A.copy(), D.copy()
    A1[8, 5] = 0.3
    D1[8, 5] = D[8, 5] / A[8, 5] * 0.3
    out3, gd, ga = _gpu(D1, A1, N, cam, 0.5, 0.1, INF, 1.0, dev)
    ref = NR.loss_and_grads(D1, A1, N, cam, 0.5, 0.1, INF, 1.0)
    assert _count(out3, W, H) == full - 5 == ref[3]
    assert NR.rel(out3, ref[0]) <= NR.B_OUT3 and NR.grad_ratio(gd, ref[1]) <= NR.B_GRADS
    assert gd[8, 5] == 0 and ga[8, 5] == 0                 # its neighbours are unsupervised: nothing flows into it
    # a corner of the interior removes only what lies inside
    A1 = A.copy()
    A1[0, 0] = 0.1
    assert _count(_gpu(D, A1, N, cam, 0.5, 0.1, INF, 1.0, dev)[0], W, H) == full
    A1[1, 0] = 0.1
    assert _count(_gpu(D, A1, N, cam, 0.5, 0.1, INF, 1.0, dev)[0], W, H) == full - 1
    # normal_min: the pixels whose |N| / A was set below it
    N3 = N.copy()
    for y, x in ((3, 4), (9, 9), (15, 14)):
        N3[:, y, x] *= 0.05 / np.linalg.norm(N3[:, y, x]) * A[y, x]
    assert _count(_gpu(D, A, N3, cam, 0.5, 0.1, INF, 1.0, dev)[0], W, H) == full - 3
    assert _count(_gpu(D, A, N3, cam, 0.5, 0.04, INF, 1.0, dev)[0], W, H) == full
    # S is counted behind the |N| gate: the mean is over the supervised pixels only
    ref = NR.loss_and_grads(D, A, N3, cam, 0.5, 0.1, INF, 1.0)
    assert NR.rel(_gpu(D, A, N3, cam, 0.5, 0.1, INF, 1.0, dev)[0], ref[0]) <= NR.B_OUT3


def test_a_depth_step_removes_the_pixels_either_side_of_it(gpu_device):
    W, H = 16, 17
    D, A, N, cam, _ = NR.plane_case(W, H)
    D = D.copy()
    D[:, 9:] *= 1.5
    assert _count(_gpu(D, A, N, cam, 0.5, 0.1, 0.05, 1.0, gpu_device)[0], W, H) == (W - 4) * (H - 2)
    assert _count(_gpu(D, A, N, cam, 0.5, 0.1, INF, 1.0, gpu_device)[0], W, H) == (W - 2) * (H - 2)


def test_a_nan_silhouette_stays_inside_its_own_gate(gpu_device):
    W, H = 16, 17
    D, A, N, cam = NR.loss_case(W, H)
    A2 = A.copy()
    A2[8, 5] = np.nan
    out3, gd, ga = _gpu(D, A2, N, cam, 0.5, 0.1, INF, 1.0, gpu_device)
    ref = NR.loss_and_grads(D, A2, N, cam, 0.5, 0.1, INF, 1.0)
    assert _count(out3, W, H) == (W - 2) * (H - 2) - 5 == ref[3]
    assert np.isfinite(out3).all() and np.isfinite(gd).all() and np.isfinite(ga).all()
    assert NR.rel(out3, ref[0]) <= NR.B_OUT3 and NR.grad_ratio(gd, ref[1]) <= NR.B_GRADS
    assert NR.grad_ratio(ga, ref[2]) <= NR.B_GRADS


# ---- every element written, determinism ---------------------------------------------------------------------------------
def test_every_gradient_element_is_written_and_runs_repeat(gpu_device):
    dev = gpu_device
    W, H = 257, 3
    D, A, N, cam = NR.loss_case(W, H)
    d, a, n = (torch.from_numpy(x).to(dev) for x in (D, A, N))
    L = G.lib()
    nbytes = int(L.gsr_normal_consistency_workspace(H, W))
    runs = []
    for _ in range(2):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        out3, gd, ga = (torch.full((k * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32) for k in (3, W * H, W * H))
        _capi._check(L.gsr_normal_consistency_loss(H, W, _capi._ptr(d), _capi._ptr(a), _capi._ptr(n), *cam, 0.5, 0.1, 0.05, 0.7,
                                                   _capi._ptr(out3), _capi._ptr(gd), _capi._ptr(ga), _capi._ptr(ws), nbytes,
                                                   _capi._stream()))
        for t in (out3, gd, ga):
            assert not (t.view(torch.int32) == -1).any()
        runs.append(torch.cat([out3, gd, ga]).view(torch.int32).clone())
    assert runs[0].any() and torch.equal(runs[0], runs[1])
    # the border pixels of the image receive a gradient too (they are the far ends of their neighbours' differences),
    # the four corners never
    g = runs[0][3:3 + W * H].view(H, W)
    assert g[0, 1:-1].any() and not g[0, 0] and not g[0, -1] and not g[-1, 0] and not g[-1, -1]


# ---- the autograd Function ------------------------------------------------------------------------------------------------
def test_the_upstream_scalar_scales_the_gradients_bit_for_bit(gpu_device):
    dev = gpu_device
    W, H = 37, 23
    D, A, N, cam = NR.loss_case(W, H)
    K = torch.tensor([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], dtype=torch.float64)
    _, gd1, ga1 = _gpu(D, A, N, cam, 0.5, 0.1, INF, 0.7, dev)
    d = torch.from_numpy(D).to(dev).requires_grad_(True)
    a = torch.from_numpy(A).to(dev)[None].requires_grad_(True)          # [1, H, W] as render returns it
    loss = G.normal_consistency_loss(d, a, torch.from_numpy(N).to(dev), K, lambda_=0.7, normal_min=0.1)
    (loss * 0.25).backward()
    assert a.grad.shape == (1, H, W)
    assert np.array_equal(d.grad.cpu().numpy(), gd1 * np.float32(0.25)) and np.array_equal(a.grad[0].cpu().numpy(), ga1 * np.float32(0.25))
    assert np.abs(gd1).max() > 0 and np.abs(ga1).max() > 0
    with pytest.raises(TypeError):
        G.normal_consistency_loss(d, a, torch.from_numpy(N).to(dev), K)      # lambda_ and normal_min have no default


def test_only_the_inputs_that_ask_receive_a_gradient(gpu_device):
    dev = gpu_device
    D, A, N, cam = NR.loss_case(16, 17)
    K = torch.tensor([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], dtype=torch.float64)
    both = _gpu(D, A, N, cam, 0.5, 0.1, INF, 0.7, dev)
    only_d = _gpu(D, A, N, cam, 0.5, 0.1, INF, 0.7, dev, grads=(True, False))
    none = _gpu(D, A, N, cam, 0.5, 0.1, INF, 0.7, dev, grads=(False, False))
    assert only_d[2] is None and np.array_equal(only_d[1], both[1]) and np.array_equal(only_d[0], both[0])
    assert none[1] is None and none[2] is None and np.array_equal(none[0], both[0])
    d = torch.from_numpy(D).to(dev).requires_grad_(True)
    a = torch.from_numpy(A).to(dev)
    G.normal_consistency_loss(d, a, torch.from_numpy(N).to(dev), K, lambda_=0.7, normal_min=0.1).backward()
    assert a.grad is None and np.array_equal(d.grad.cpu().numpy(), both[1])
