"""Plain-Torch / numpy restatement of the evaluation pass (csrc/metrics.hip) on the CPU, the bars its kernels are held to
and the inputs they are held on.  Nothing here imports the package.  SSIM and L1 are loss_ref.py's (imported).

    mse_c = mean over H W of (x - y)^2 in channel c        x = img, y = gt, [C][H][W]
    psnr  = mean_c 20 log10(1 / sqrt(mse_c))                (gaussian_splatting::psnr, loss_utils.cuh:89-93, as it stands:
                                                            the MEAN OF THE PER-CHANNEL PSNRs, not the PSNR of the pooled error)
    mse   = mean_c mse_c
    u8(x)   = trunc(clamp(x * 255, 0, 255)), one float32 multiply           (tensor2CvMat3X, lioOptimization.cpp:2121)
    u8d(d)  = saturate(round_half_even(d * (255 / max_depth))), factor and product in float32    (:2155-2158, convertTo)

Run in float64 `metrics` is the truth; run in float32 it is the yardstick e_ref = |float32 - float64|.  The bar of every
compared number is max(2 e_ref, floor), floor = K 2^-23 magnitude, as in loss_ref.py.  A rounding is half a unit
(2^-24 relative); K is in units of 2^-23 = two roundings.  Counted from csrc/metrics.hip before any kernel ran:

  sum (x - y)^2 of a channel (k_metrics_forward).  d = x - y: one rounding of d, i.e. two of d^2.  A thread folds its (at
  most 8) squares into its sum with one fused multiply-add each: 8 roundings of the running sum.  A wave's butterfly has 6
  levels, the four waves 2 more.  Every term is non-negative, so nothing cancels and every rounding is relative to the sum:
  2 + 8 + 6 + 2 = 18 roundings.  The partials are added in float64, divided by H W in float64 (nothing at this scale).
                                                                                                      K_SQ = 18 / 2 = 9
  mse    the mean of the mse_c in float64 and ONE narrowing: 19 roundings                                   K_MSE = 10
  psnr   psnr_c = -10 log10(mse_c): a relative error r of mse_c moves it by (10 / ln 10) r, whatever its size (a sum of
         non-negative terms has no cancellation), and so the mean over the channels.  sqrt, the division, log10 and the
         mean are float64; the result is narrowed once: half a unit of |psnr|.
             floor(psnr) = 2^-23 ((10 / ln 10) K_SQ + 0.5 |psnr|)          (= 39.1 + 0.5 |psnr| units: ABSOLUTE, in dB)
         An infinite psnr (a channel with mse_c == 0: x - y is exact there, so the kernel's sum is exactly 0 too) is
         compared for equality.
  l1     loss_ref.py's K_L1 = 10 (the same sum, the same finalize)                               floor = K_L1 E l1
  ssim   loss_ref.py's floor: mean(carried) + (K_SSIM + K_SUM) E mean|SSIM| (`loss_ref.floors`, unchanged: the same
         arithmetic in the same order)

The float32 restatement itself (CPU; test_metrics_ref.py repeats it): its psnr is within 0.8 * 2^-23 * max(1, |psnr|) of
float64 on shapes from (3, 1, 1) to (3, 1080, 1920) at amplitudes 1e-4 ... 1, inside every bar above.
"""
import functools
import math

import numpy as np
import torch

import loss_ref as R

EPS32 = R.EPS32
K = dict(sq=9, mse=10, l1=R.K["l1"])
DB_PER_REL = 10.0 / math.log(10.0)


# ---- the restatement -----------------------------------------------------------------------------------------------
def psnr_parts(img, gt, dtype):
    """(psnr, mse, [mse_c]) as python floats from an evaluation in `dtype`: loss_utils.cuh:89-93 line for line."""
    x, y = img.detach().to(dtype), gt.detach().to(dtype)
    squared_diff = (x - y).pow(2)
    mse_val = squared_diff.view(x.size(0), -1).mean(1, True)
    psnr = (20.0 * torch.log10(1.0 / mse_val.sqrt())).mean()
    return float(psnr), float(mse_val.mean()), [float(v) for v in mse_val.reshape(-1)]


def psnr_pooled(img, gt, dtype=torch.float64):
    """What the reference does NOT compute: the PSNR of the error pooled over the channels."""
    x, y = img.detach().to(dtype), gt.detach().to(dtype)
    return float(20.0 * torch.log10(1.0 / (x - y).pow(2).mean().sqrt()))


def metrics(img, gt, w1d, dtype):
    """{psnr, ssim, l1, mse, mse_c}: the four outputs of gsr_image_metrics from an evaluation in `dtype`."""
    p, mse, mse_c = psnr_parts(img, gt, dtype)
    r = R.loss_parts(img, gt, w1d, 1.0, dtype, want_grad=False)
    return dict(psnr=p, ssim=r["ssim"], l1=r["l1"], mse=mse, mse_c=mse_c)


def floors(img, gt, w1d, r64):
    fl = R.floors(img, gt, w1d, 1.0)
    psnr = r64["psnr"]
    return dict(psnr=EPS32 * (DB_PER_REL * K["sq"] + 0.5 * abs(psnr)) if math.isfinite(psnr) else 0.0,
                ssim=fl["ssim"], l1=fl["l1"], mse=K["mse"] * EPS32 * r64["mse"])


def bars(r64, r32, fl):
    """{name: (e_ref, bar)}; an infinite psnr has no bar (it is compared for equality)."""
    out = {}
    for k in ("psnr", "ssim", "l1", "mse"):
        if not math.isfinite(r64[k]):
            assert r32[k] == r64[k], (k, r32[k], r64[k])
            out[k] = (0.0, 0.0)
            continue
        e = abs(r32[k] - r64[k])
        out[k] = (e, max(2 * e, fl[k]))
    return out


def ratios(got, r64, bar):
    """{name: (err, e_ref, bar, err / bar)}; got: the four floats of out4 in order."""
    res = {}
    for k, v in zip(("psnr", "ssim", "l1", "mse"), got):
        v = float(v)
        if not math.isfinite(r64[k]):
            res[k] = (0.0, 0.0, 0.0, 0.0 if v == r64[k] else math.inf)
            continue
        err = abs(v - r64[k])
        assert math.isfinite(err), (k, v)
        res[k] = (err, bar[k][0], bar[k][1], (err / bar[k][1]) if err else 0.0)
    return res


# ---- the two 8-bit conversions --------------------------------------------------------------------------------------
def to_u8(img, bgr=True):
    """tensor2CvMat3X: [3,H,W] float32 CPU -> uint8 [H,W,3].  NaN is undefined there (and in Torch's cast): callers
    that hold NaN assert those pixels themselves; here they come out as whatever int32(NaN) is."""
    assert img.dtype == torch.float32
    t = img.permute(1, 2, 0).mul(255).clamp(0, 255).to(torch.int32).to(torch.uint8)   # (truncation toward zero)
    return (t.flip(2) if bgr else t).contiguous()


def depth_to_u8(depth, max_depth):
    """cv::Mat::convertTo(CV_8U) of depth * (255.0f / maxDepth) as OpenCV documents it (saturate_cast<uchar> of the
    value rounded half to even), numpy float32 throughout; NaN -> 0 (the kernel's choice)."""
    d = depth.detach().reshape(depth.shape[-2], depth.shape[-1]).numpy().astype(np.float32)
    scale = np.float32(255.0) / np.float32(max_depth)
    v = d * scale
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v), 0.0, 255.0)
    return torch.from_numpy(np.where(np.isnan(r), 0.0, r).astype(np.uint8))


def _neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


SPECIALS = np.array([0.5, 254.9999 / 255.0, -0.0, 0.0, -1e-30, -0.25, -7.0, 1.0, 1.0000001, 1.5, 300.0, np.inf, -np.inf,
                     1e-45, 3e38], np.float32)


def unit_pool():
    """Every k / 255 with its two float neighbours and the special values: the inputs of k_pack_image_u8 (float32)."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    return np.concatenate([_neighbours(k), SPECIALS]).astype(np.float32)


def depth_pool():
    """Depths at max_depth = 255 (factor exactly 1): every k, every tie k + 0.5 and their float neighbours, specials."""
    k = np.arange(256, dtype=np.float32)
    return np.concatenate([_neighbours(k), _neighbours(k + np.float32(0.5)),
                           np.array([-0.0, -0.5, -0.50001, -3.0, 255.5, 256.0, 1e9, np.inf, -np.inf, 1e-45], np.float32)])


# ---- inputs --------------------------------------------------------------------------------------------------------
def tiny_noise(shape, seed=0):
    """Noise of amplitude 1e-4 on the image: PSNR near 80 dB."""
    g = R._gen(shape, seed + 11)
    gt = torch.rand(shape, generator=g)
    return gt + 1e-4 * torch.randn(shape, generator=g), gt


def decades(shape, seed=0):
    """A constant offset of 1e-1, 1e-3, 1e-5 on channels 0, 1, 2 (and round again): per-channel PSNRs of 20, 60 and
    100 dB, mean 60, against 24.8 dB for the pooled error."""
    g = R._gen(shape, seed + 12)
    gt = 0.1 + 0.8 * torch.rand(shape, generator=g)
    off = torch.tensor([10.0 ** -(1 + 2 * (c % 3)) for c in range(shape[0])], dtype=torch.float64)[:, None, None]
    return (gt.double() + off).float(), gt


def identical(shape, seed=0):
    gt = R.noise(shape, seed + 13)[1]
    return gt.clone(), gt


def one_identical_channel(shape, seed=0):
    img, gt = R.noise(shape, seed + 14)
    img[0] = gt[0]
    return img, gt


GENERATORS = dict(noise=R.noise, dark=R.dark, bright=R.bright, edges=R.edges, tiny_noise=tiny_noise, decades=decades,
                  identical=identical, one_identical_channel=one_identical_channel)
_NAMES = tuple(GENERATORS)

# (1, 1, 1); H or W in {1, 5, 11} (the halo); W in {53, 54, 55, 108, 109} and H in {31, 32, 33, 64, 65} (the 54 x 32 work
# unit); C in {1, 3, 4}; (1, 1, 55404): 1026 partials in ONE channel, past the 1024 threads of k_metrics_finalize
SHAPES = [(1, 1, 1), (3, 1, 53), (1, 5, 54), (3, 11, 55), (4, 31, 108), (3, 32, 109), (1, 33, 1), (3, 64, 5), (4, 65, 11),
          (3, 33, 55), (1, 65, 109), (1, 1, 55404)]
BOTH_SEAMS = (3, 33, 55)


def _cases():
    out = []
    for i, s in enumerate(SHAPES):                 # every shape with two generators (rotating) ...
        out += [(_NAMES[i % 8], s), (_NAMES[(i + 3) % 8], s)]
    out += [(g, BOTH_SEAMS) for g in _NAMES]       # ... and every generator where both axes cross a seam
    out += [("noise", (1, 1, 55404)), ("decades", (3, 1, 55404))]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


@functools.lru_cache(maxsize=8)
def _shared(name, shape):
    img, gt = GENERATORS[name](shape)
    img, gt = img.float().contiguous(), gt.float().contiguous()
    w = R.reference_window_1d()
    r64, r32 = metrics(img, gt, w, torch.float64), metrics(img, gt, w, torch.float32)
    fl = floors(img, gt, w, r64)
    return dict(img=img, gt=gt, w=w, r64=r64, r32=r32, floors=fl, bar=bars(r64, r32, fl))


def case(name, shape):
    """The cached reference is shared; the inputs a test may upload are copies."""
    c = _shared(name, tuple(shape))
    return dict(c, img=c["img"].clone(), gt=c["gt"].clone(), w=c["w"].clone())
