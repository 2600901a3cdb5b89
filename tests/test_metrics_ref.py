"""CPU tests of tests/metrics_ref.py: the restatement of the evaluation pass is anchored on closed forms, so that the
GPU tests compare the kernels with something that is itself held."""
import math

import numpy as np
import pytest
import torch

import loss_ref as R
import metrics_ref as M


@pytest.mark.parametrize("delta", [0.25, 1e-2, 1e-4])
def test_constant_offset_gives_minus_20_log10_delta(delta):
    gt = torch.rand((3, 7, 9), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    p, mse, mse_c = M.psnr_parts(gt + delta, gt, torch.float64)
    assert abs(p - (-20.0 * math.log10(delta))) < 1e-6
    assert all(abs(m - delta * delta) < 1e-9 * delta * delta + 1e-24 for m in mse_c) and abs(mse - delta * delta) < 1e-12


def test_per_channel_mean_is_not_the_pooled_psnr():
    gt = torch.rand((3, 6, 5), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    img = gt + torch.tensor([1e-1, 1e-3, 1e-5], dtype=torch.float64)[:, None, None]
    p, _, mse_c = M.psnr_parts(img, gt, torch.float64)
    assert abs(p - (20.0 + 60.0 + 100.0) / 3.0) < 1e-5          # the mean of the per-channel PSNRs ...
    pooled = M.psnr_pooled(img, gt)
    assert abs(pooled - (-10.0 * math.log10((1e-2 + 1e-6 + 1e-10) / 3.0))) < 1e-6
    assert p - pooled > 10.0                                     # ... which the pooled formula misses by 35 dB
    img32, gt32 = M.decades((3, 33, 55))
    assert abs(M.psnr_parts(img32, gt32, torch.float64)[0] - 60.0) < 0.1
    assert M.psnr_parts(img32, gt32, torch.float64)[0] - M.psnr_pooled(img32, gt32) > 10.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identical_images_and_one_identical_channel_are_infinite(dtype):
    for gen in (M.identical, M.one_identical_channel):
        img, gt = gen((3, 5, 11))
        p, mse, mse_c = M.psnr_parts(img, gt, dtype)
        assert p == math.inf and mse_c[0] == 0.0 and math.isfinite(mse)
    img, gt = M.identical((3, 5, 11))
    assert abs(M.metrics(img, gt, R.reference_window_1d(), torch.float64)["ssim"] - 1.0) < 1e-12


@pytest.mark.parametrize("shape,amp", [((3, 1, 1), 1.0), ((3, 5, 11), 1e-4), ((3, 33, 55), 1e-2), ((1, 1, 55404), 1.0),
                                       ((3, 512, 640), 1e-4), ((3, 1080, 1920), 1.0)])
def test_float32_yardstick_is_inside_the_psnr_floor(shape, amp):
    """The float32 restatement's own psnr error: within 0.8 * 2^-23 * max(1, |psnr|), and inside the counted floor."""
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(shape, generator=g)
    img = gt + amp * (torch.rand(shape, generator=g) - 0.5)
    p64, _, _ = M.psnr_parts(img, gt, torch.float64)
    p32, _, _ = M.psnr_parts(img, gt, torch.float32)
    e = abs(p32 - p64)
    print("shape", shape, "amp", amp, "psnr", p64, "e_ref / (2^-23 max(1, |psnr|)) = %.3f" % (e / (M.EPS32 * max(1.0, abs(p64)))))
    assert e <= 0.8 * M.EPS32 * max(1.0, abs(p64))
    assert e <= M.EPS32 * (M.DB_PER_REL * M.K["sq"] + 0.5 * abs(p64))


def test_every_gpu_case_has_a_reference_and_positive_bars():
    for name, shape in M.CASES:
        if shape[1] * shape[2] > 6000:
            continue                                   # (the GPU module builds these; here: the small ones)
        c = M.case(name, shape)
        for k in ("psnr", "ssim", "l1", "mse"):
            e, bar = c["bar"][k]
            assert (bar > 0 and bar >= 2 * e) or not math.isfinite(c["r64"][k]) or c["r64"][k] == 0.0, (name, shape, k)
        if name in ("identical", "one_identical_channel"):
            assert c["r64"]["psnr"] == math.inf
        if name == "tiny_noise" and shape[1] * shape[2] > 100:
            assert 75.0 < c["r64"]["psnr"] < 85.0


def test_truncation_table():
    x = torch.tensor([0.5, np.float32(254.9999 / 255.0), -0.0, -0.25, -7.0, 1.0, 1.5, 300.0, math.inf, -math.inf, 0.0,
                      1.0 / 255.0], dtype=torch.float32)
    want = [127, 254, 0, 0, 0, 255, 255, 255, 255, 0, 0, 1]
    img = x[None, None, :].expand(3, 1, -1).contiguous()
    got = M.to_u8(img, bgr=False)
    assert got.shape == (1, len(want), 3) and got[0, :, 0].tolist() == want and got[0, :, 2].tolist() == want
    # channel order: plane c lands in byte c (RGB) or 2 - c (BGR)
    planes = torch.stack([torch.full((2, 3), v / 255.0) for v in (10.0, 20.0, 30.0)])
    assert M.to_u8(planes, bgr=False)[0, 0].tolist() == [10, 20, 30] and M.to_u8(planes, bgr=True)[0, 0].tolist() == [30, 20, 10]
    # every k / 255 comes back as k: float32(k / 255) * 255 never lands below k
    k = torch.arange(256, dtype=torch.float32)
    assert M.to_u8((k / 255.0)[None, None, :].expand(3, 1, -1).contiguous(), bgr=False)[0, :, 1].tolist() == list(range(256))


def test_half_even_table():
    d = torch.tensor([[0.5, 1.5, 2.5, 254.5, 255.5, -0.0, -0.5, -3.0, 256.0, math.inf, -math.inf, math.nan, 0.49999997,
                       0.50000006]], dtype=torch.float32)
    assert M.depth_to_u8(d, 255.0)[0].tolist() == [0, 2, 2, 254, 255, 0, 0, 0, 255, 255, 0, 0, 0, 1]
    # the factor is formed in float32: 255 / 50 = 5.1 is not a float, so 2.5 * 5.1f = 12.75 -> 13 and 10 * 5.1f -> 51
    assert M.depth_to_u8(torch.tensor([[2.5, 10.0, 50.0, 60.0]]), 50.0)[0].tolist() == [13, 51, 255, 255]


def test_pools_hold_what_the_gpu_tests_promise():
    u = M.unit_pool()
    assert u.dtype == np.float32 and len(u) == 3 * 256 + len(M.SPECIALS)
    for k in range(256):
        v = np.float32(k) / np.float32(255.0)
        assert v in u and np.nextafter(v, np.float32(2)) in u and np.nextafter(v, np.float32(-1)) in u
    assert not np.isnan(u).any() and not np.isnan(M.depth_pool()).any()    # (NaN is asserted apart, not through Torch)
