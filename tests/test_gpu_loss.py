"""GPU tests of the fused photometric loss (csrc/loss.hip; SURVEY.md 8(f) "next" row 2) against a plain
PyTorch f32 restatement of the reference's l1_loss / ssim (include/gs/gs/loss_utils.cuh:11-13, 43-70), built from
grouped conv2d exactly as the reference does, with the reference's own (asymmetric) window."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gs_livm_amd as G

pytestmark = pytest.mark.gpu
C1, C2 = 0.01 * 0.01, 0.03 * 0.03


def ref_ssim(img1, img2, w1d):
    ch = img1.shape[0]
    window = (w1d[:, None] @ w1d[None, :])[None, None].expand(ch, 1, 11, 11).contiguous()
    conv = lambda x: F.conv2d(x[None], window, padding=5, groups=ch)[0]  # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    s1 = conv(img1 * img1) - mu1 * mu1
    s2 = conv(img2 * img2) - mu2 * mu2
    s12 = conv(img1 * img2) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return m.mean()


def ref_loss(img, gt, w1d, lam):
    return (1 - lam) * (img - gt).abs().mean() + lam * (1 - ref_ssim(img, gt, w1d))


def ref_loss_f64(img, gt, w1d, lam):
    """ref_loss evaluated in float64 on the CPU: loss and d loss / d img, free of the f32 convolution's own rounding
    and backend choices."""
    x = img.detach().double().cpu().requires_grad_(True)
    want = ref_loss(x, gt.detach().double().cpu(), w1d.double().cpu(), lam)
    (g,) = torch.autograd.grad(want, x)
    return float(want.detach()), g


def variance_rounding_slack(img, gt, w1d, lam):
    """How far the loss may move, in f64, when sigma1, sigma2 and sigma12 carry the rounding an f32 evaluation of
    conv(x * y) - mu_x * mu_y has (2 ulp of each of the two terms).  Where the planes are flat the sigmas are ~0 and
    only C2 stays in the contrast-structure denominator, so that rounding reaches the loss amplified by 1 / C2 -- in the
    reference's own f32 formula as in any other."""
    x, y = img.detach().double().cpu(), gt.detach().double().cpu()
    ch = x.shape[0]
    w = w1d.double().cpu()
    window = (w[:, None] @ w[None, :])[None, None].expand(ch, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], window, padding=5, groups=ch)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    e11, e22, e12 = conv(x * x), conv(y * y), conv(x * y)
    s = [(e11 - mu1 * mu1).requires_grad_(True), (e22 - mu2 * mu2).requires_grad_(True),
         (e12 - mu1 * mu2).requires_grad_(True)]
    m = ((2 * mu1 * mu2 + C1) * (2 * s[2] + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s[0] + s[1] + C2))
    d = torch.autograd.grad(m.sum(), s)
    u = 2.0 ** -24
    err = [2 * u * (e11.abs() + mu1 * mu1), 2 * u * (e22.abs() + mu2 * mu2), 2 * u * (e12.abs() + (mu1 * mu2).abs())]
    return lam * float(sum((di.abs() * ei).sum() for di, ei in zip(d, err))) / m.numel()


def _check_f64(got, gg, img, gt, lam, scale_floor=0.0, value_slack=0.0):
    """The kernel's loss and gradient (gg = d got / d img) against ref_loss_f64, at the tolerances of
    test_fused_loss_matches_torch (the loss's widened by value_slack, computed in f64, where given)."""
    want, gw = ref_loss_f64(img, gt, G.reference_window_1d(), lam)
    assert abs(float(got) - want) <= 2e-6 * max(1.0, abs(want)) + value_slack, (float(got), want, value_slack)
    scale = max(float(gw.abs().max()), scale_floor)
    err = float((gg.double().cpu() - gw).abs().max())
    assert err <= 2e-5 * scale + 1e-9, (err, scale)


@pytest.mark.parametrize("shape,lam", [((3, 45, 67), 0.2), ((3, 300, 200), 0.2), ((1, 16, 16), 0.5), ((3, 9, 7), 0.0),
                                       ((3, 128, 130), 1.0),
                                       # the shapes the bench and the product run (54 x 32-pixel work units:
                                       # 1920 = 35.6 units wide, 1080 = 33.75 high; 640 x 512 = 11.9 x 16)
                                       ((3, 1080, 1920), 0.2), ((3, 512, 640), 0.2),
                                       # edges of the 54 x 32 work units and of the 11-tap halo: H or W in
                                       # {1, 2, 10, 11, 53, 54, 55}, H in {31, 32, 33}
                                       ((3, 1, 55), 0.2), ((3, 2, 54), 0.2), ((3, 10, 53), 0.2), ((3, 11, 11), 0.2),
                                       ((3, 53, 2), 0.2), ((3, 54, 1), 0.2), ((3, 55, 10), 0.2), ((1, 1, 1), 0.2),
                                       ((3, 31, 64), 0.2), ((3, 32, 108), 0.2), ((3, 33, 55), 0.2)])
def test_fused_loss_matches_torch(shape, lam, gpu_device):
    gen = torch.Generator().manual_seed(shape[1])
    img = torch.rand(shape, generator=gen).to(gpu_device).requires_grad_(True)
    gt = torch.rand(shape, generator=gen).to(gpu_device)
    # a structured target makes SSIM non-trivial
    gt = (0.6 * gt + 0.4 * img.detach().roll(1, 2)).clamp(0, 1)
    w = G.reference_window_1d()
    want = ref_loss(img, gt, w.to(gpu_device), lam)
    (gw,) = torch.autograd.grad(want, img)
    img2 = img.detach().clone().requires_grad_(True)
    got = G.photometric_loss(img2, gt, lam)
    (gg,) = torch.autograd.grad(3.0 * got, img2)  # upstream scale is honoured
    assert abs(float(got) - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
    scale = float(gw.abs().max())
    assert float((gg / 3.0 - gw).abs().max()) <= 2e-5 * scale + 1e-9
    _check_f64(got, gg / 3.0, img, gt, lam)


@pytest.mark.parametrize("shape,lam", [((3, 54, 55), 0.0), ((3, 54, 55), 0.2), ((3, 33, 11), 1.0), ((1, 2, 1), 0.2)])
def test_fused_loss_image_equals_target(shape, lam, gpu_device):
    """img == gt bit for bit: the L1 term takes the sign(0) = 0 branch (its gradient is exactly zero), SSIM is 1 and
    its gradient vanishes in exact arithmetic, so what the kernel returns is rounding alone.  The gradient is held to
    the f64 one relative to the scale (1 - lam + lam) / numel of a unit L1 gradient, since the exact gradient is 0."""
    gen = torch.Generator().manual_seed(shape[1] + shape[2])
    gt = torch.rand(shape, generator=gen).to(gpu_device)
    img = gt.clone().requires_grad_(True)
    got = G.photometric_loss(img, gt, lam)
    (gg,) = torch.autograd.grad(got, img)
    if lam == 0.0:
        assert float(got) == 0.0 and not gg.any()
    _check_f64(got, gg, img, gt, lam, scale_floor=1.0 / img.numel())


@pytest.mark.parametrize("shape", [(3, 54, 55), (3, 33, 11), (1, 1, 1)])
def test_fused_loss_constant_planes(shape, gpu_device):
    """Constant image and target planes (zero variance: SSIM reduces to its luminance term with C2 / C2), and a
    constant image against a varying target; each against the f64 reference.  The loss's bar is widened by
    variance_rounding_slack: measured at (3, 54, 55), 0.25 against 0.75, the kernel is 8.7e-6 off the f64 loss
    (the slack computed for it: 2.3e-5)."""
    gen = torch.Generator().manual_seed(shape[2])
    for a, b in ((0.25, 0.75), (0.5, None)):
        img = torch.full(shape, a).to(gpu_device).requires_grad_(True)
        gt = torch.full(shape, b) if b is not None else torch.rand(shape, generator=gen)
        gt = gt.to(gpu_device)
        got = G.photometric_loss(img, gt, 0.2)
        (gg,) = torch.autograd.grad(got, img)
        _check_f64(got, gg, img, gt, 0.2,
                   value_slack=variance_rounding_slack(img, gt, G.reference_window_1d(), 0.2))


def test_symmetric_window_and_determinism(gpu_device):
    gen = torch.Generator().manual_seed(5)
    img = torch.rand((3, 100, 90), generator=gen).to(gpu_device).requires_grad_(True)
    gt = torch.rand((3, 100, 90), generator=gen).to(gpu_device)
    x = torch.arange(11, dtype=torch.float32) - 5
    w = torch.exp(-x * x / 4.5)
    w = w / w.sum()  # the centred window of the original SSIM code
    want = ref_loss(img, gt, w.to(gpu_device), 0.2)
    a = G.photometric_loss(img, gt, 0.2, window11=w)
    b = G.photometric_loss(img, gt, 0.2, window11=w)
    assert float(a) == float(b)  # fixed-order reduction
    assert abs(float(a) - float(want)) <= 2e-6
