"""Plain-Torch restatement of k_init_gaussians (csrc/growth.hip) with the dtype as a parameter, its bars and its inputs.
Nothing here imports the package.

    scaling = log(sqrt(diag(cov) * scale_factor))        f_dc = (rgb / 255 - 0.5) / C0,  C0 narrowed to float32 first
    xyz copied; rotation = (1, 0, 0, 0); opacity = 0; f_rest = 0

Bars, per element: max(2 e_ref, floor), e_ref = |float32 restatement - float64| (loss_ref.py's convention: a rounding is
2^-24 relative, E = 2^-23 is two).
  scaling  p = diag * s is rounded once: relative 2^-24, or 2^-150 / |p| where p is subnormal.  The root halves a relative
           error and adds its own rounding (correctly rounded: 2^-24); the logarithm turns the RELATIVE error of its
           argument into an ABSOLUTE one -- which is all that is left where the value is near 0, p near 1.  Its own error:
           the device logf is the OpenCL built-in of the device library, whose bound is 3 ulp of the infinitely precise
           result (OpenCL C specification, relative error of log, full profile); an ulp is at most E |value|.  (A first
           count of 1 ulp was wrong: logf(sqrtf(p)) measures up to 1.5 E |value| on an MI355X at |value| in 30 ... 44,
           inside the documented bound; float32 Torch on the CPU is within 0.5.)
               floor = 0.5 max(2^-24, 2^-150 / |p|) + 2^-24 + 3 E |value|
  f_dc     the quotient rgb / 255 (one rounding of |rgb / 255|, carried through the subtraction unchanged and divided by
           C0), the subtraction and the division (two roundings of the value):
               floor = E (0.5 |rgb / 255| / C0 + |value|)
Zero, negative and overflowing products give -inf, NaN and +inf: there, and wherever the float32 restatement is not
finite, the IEEE CLASS is compared with the float32 restatement (the reference's arithmetic) and no value.
"""
import numpy as np
import torch

C0 = float(np.float32(0.28209479177387814))
E = 2.0 ** -23
K_LOG = 3
NS = (1, 255, 256, 257, 4097)
MS = (1, 2, 3, 4, 9, 16)
LOS = (0, 1, 2, 3, 257)
SCALES = (0.5, 1.7, 4.0)


def init_ref(covs, rgbs, scale_factor, dtype):
    """(scaling [n,3], f_dc [n,3]) in `dtype`, returned as float64."""
    s = float(np.float32(scale_factor))
    diag = covs.to(dtype).diagonal(0, -2, -1)
    scaling = torch.log(torch.sqrt(diag * s))
    fdc = (rgbs.to(dtype) / 255.0 - 0.5) / C0
    return scaling.double(), fdc.double()


def floors(covs, rgbs, scale_factor):
    s = float(np.float32(scale_factor))
    p = covs.double().diagonal(0, -2, -1) * s
    v, f = init_ref(covs, rgbs, scale_factor, torch.float64)
    rel = torch.maximum(torch.full_like(p, 2.0 ** -24), 2.0 ** -150 / p.abs().clamp(min=1e-300))
    fs = 0.5 * rel + 2.0 ** -24 + K_LOG * E * torch.nan_to_num(v.abs(), nan=0.0, posinf=0.0, neginf=0.0)
    ff = E * (0.5 * (rgbs.double() / 255.0).abs() / C0 + f.abs())
    return fs, ff


def ieee_class(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    t = t.double()
    return torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3


def judge(got_scaling, got_fdc, covs, rgbs, scale_factor):
    """{scaling, f_dc: (max err, max e_ref, worst err / bar)} over every element whose float32 restatement is finite;
    asserts the IEEE class of EVERY element against the float32 restatement."""
    r64, r32 = init_ref(covs, rgbs, scale_factor, torch.float64), init_ref(covs, rgbs, scale_factor, torch.float32)
    fl = floors(covs, rgbs, scale_factor)
    res = {}
    for name, got, a64, a32, f in zip(("scaling", "f_dc"), (got_scaling, got_fdc), r64, r32, fl):
        got = got.double().cpu().reshape(a64.shape)
        assert torch.equal(ieee_class(got), ieee_class(a32)), "%s: IEEE classes differ from the float32 restatement" % name
        ok = torch.isfinite(a32) & torch.isfinite(a64)
        err, e = (got - a64).abs()[ok], (a32 - a64).abs()[ok]
        bar = torch.maximum(2 * e, f[ok])
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
        res[name] = (float(err.max()), float(e.max()), float(ratio.max())) if err.numel() else (0.0, 0.0, 0.0)
    return res


def _f32_from_bits(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def cloud(n, seed, scale_factor):
    """xyz [n,3], covs [n,3,3], rgbs [n,3], float32 CPU.  Diagonals 10^U(-30, 30) / s; every off-diagonal element a
    distinct value of its own (a kernel that reads the wrong element cannot agree); rows 0..15 (cyclically, where n
    allows) carry the special cases: a product of exactly 1, subnormal, +0, -0, negative, overflowing (3e38 at s > 1),
    2^-126 and FLT_MAX / s diagonals; rgb 0, 255, fractional and above 255.  xyz holds -0.0, subnormals and NaNs with
    payloads, compared as bits."""
    g = torch.Generator().manual_seed(104729 * seed + n)
    s = float(np.float32(scale_factor))
    diag = (10.0 ** (-30 + 60 * torch.rand((n, 3), generator=g, dtype=torch.float64)) / s).float()
    covs = (torch.rand((n, 3, 3), generator=g) * 2 - 1) * 7.0 + torch.arange(9.0).view(1, 3, 3)
    special = [1.0 / s, 1e-40, 0.0, -0.0, -2.5, 3e38, 2.0 ** -126, 3.4028234663852886e38 / s, 1.0000001 / s, 1e-45,
               float(np.float32(2.0 ** -149)), 0.99999994 / s, 2.0 / s, 1e30, 1e-30, 6e-39]
    for i in range(min(n, 64)):
        diag[i, i % 3] = special[(i // 3 + i) % 16] if n > 1 else special[0]
    covs.diagonal(0, -2, -1).copy_(diag)
    rgbs = torch.randint(0, 256, (n, 3), generator=g).float()
    frac = torch.rand((n, 3), generator=g)
    rgbs = torch.where(frac < 0.3, rgbs + frac, rgbs)
    for i, v in enumerate((0.0, 255.0, 127.5, 300.5, 1e-3, 254.99998)):
        if i < n:
            rgbs[i, i % 3] = v
    xyz = (torch.rand((n, 3), generator=g) * 6 - 3)
    bits = [0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000]
    sp = _f32_from_bits(bits)
    flat = xyz.view(-1)
    for i in range(min(flat.numel(), 24)):
        if i % 3 != 1 or n == 1:
            flat[i] = sp[i % 8]
    return xyz, covs, rgbs


def bits(t):
    return t.contiguous().view(torch.int32)
