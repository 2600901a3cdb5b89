"""Float64 truth and bars of the exposure-compensated photometric loss (csrc/exposure.hip), on the CPU.  Imports
loss_ref and nothing from the package.

    x'(p) = fma(g_c, x(p), b_c)          exposure[c] = (g_c, b_c), float32
    L     = loss_ref's L at (x', gt)     zero padding of x' (outside the image x' is 0, NOT b_c)
    G     = dL/dx'                       dL/dx = g_c G,   dL/dg_c = sum_p G x  (the ORIGINAL x),   dL/db_c = sum_p G

`compensate` restates the kernels' float32 FMA exactly: the float64 product of two float32 values is exact (48 bits),
the float64 sum with b is rounded to 53 bits and narrowed once to 24.  The two roundings equal the FMA's single one unless
the float64 sum lands on a float32 midpoint that the exact sum misses (a double-rounding tie): `ties` counts the elements
whose float64 sum is such a midpoint and was rounded to get there (test_exposure_ref.py holds it at zero for every input
used here, and checks one small case against exact rationals).  So x' is the same float32 array on both sides, and
everything loss_ref derives for (img, gt) applies unchanged to (x', gt):

  truth  loss_ref.loss_parts in float64 at (compensate(img, e), gt), x' the leaf -> {L, l1, ssim}, G64; then, in float64,
         dL/dimg = g G64,  dL/dg_c = sum G64 x,  dL/db_c = sum G64
  bars   {L, l1, ssim} and G: loss_ref.bars, unchanged (bar_G per pixel)
         dL/dimg(p)   |g_c| bar_G(p) + 2^-24 |g_c G64(p)|        (the kernel's one more multiply: half a unit of 2^-23)
         dL/dg_c      sum_p bar_G(p) |x(p)| + 2^-24 |value|      (every G off by its whole bar, all to one side; the
         dL/db_c      sum_p bar_G(p)        + 2^-24 |value|       float64 sums add nothing; one narrowing)
Worst-case sums of counts that loss_ref.py already holds: nothing new is measured.  What the kernels reach is in
DESIGN.md section 2.
"""
import functools

import torch
import torch.nn.functional as F

import loss_ref as R

HALF = 2.0 ** -24
SHAPES = [(1, 1, 1), (3, 7, 5), (3, 32, 54), (3, 33, 55), (1, 65, 109)]   # one pixel; below the window; exactly one
#                                                     work unit; one pixel past both seams; 3 x 3 units
MANY = R.MANY_PARTIALS[0]                                                # > 1024 partials per channel
GENS = ("noise", "edges", "dark", "bright")
ROWS = ((0.8, -0.05), (1.0, 0.0), (1.25, 0.1))
EXPOSURES = dict(rows=ROWS, rolled=ROWS[1:] + ROWS[:1], rolled2=ROWS[2:] + ROWS[:2],
                 negative=((-0.7, 0.9), (0.8, -0.05), (-1.25, 1.3)), identity=((1.0, 0.0),) * 3)


def exposure(key, channels):
    """[C,2] float32: the first C rows of EXPOSURES[key] (every channel its own row: a wrong channel index shows)."""
    return torch.tensor(EXPOSURES[key][:channels], dtype=torch.float32)


def compensate(img, e):
    """fma(g_c, img, b_c) in float32, restated (module docstring).  e: [C,2] float32."""
    e = torch.as_tensor(e, dtype=torch.float32).reshape(-1, 2)
    return _sum64(img, e).float()


def _sum64(img, e):
    assert img.dtype == torch.float32 and e.dtype == torch.float32
    return e[:, 0].double()[:, None, None] * img.double() + e[:, 1].double()[:, None, None]


def ties(img, e):
    """Number of elements at which narrowing the rounded float64 sum can differ from the FMA's single rounding: the
    float64 sum g x + b sits exactly on the midpoint of two float32 values AND the float64 addition was inexact (its
    error term, by two-sum, is not zero).  An exact midpoint is no hazard: both routes round it to even."""
    e = torch.as_tensor(e, dtype=torch.float32).reshape(-1, 2)
    p = e[:, 0].double()[:, None, None] * img.double()           # exact
    b = e[:, 1].double()[:, None, None].expand_as(p)
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)                               # two-sum: s + err == p + b exactly
    low = s.contiguous().view(torch.int64) & ((1 << 29) - 1)      # the 29 mantissa bits float32 drops
    return int(((low == (1 << 28)) & (err != 0)).sum())


def loss64(xp, gt, w1d, lam, pad_value=None):
    """loss_ref's L as a differentiable function of x' (any dtype of xp), grouped 11 x 11 conv2d.  pad_value: None =
    zero padding; a [C] tensor = the MUTANT that pads channel c of x' with pad_value[c] (what forming x' behind the
    padding select would compute)."""
    ch = xp.shape[0]
    y = gt.to(xp.dtype)
    window = R._window(w1d.to(xp.dtype), ch)
    ypad = F.pad(y[None], (5, 5, 5, 5))

    def padded(t):
        if pad_value is None:
            return F.pad(t[None], (5, 5, 5, 5))
        inside = F.pad(torch.ones_like(t)[None], (5, 5, 5, 5))
        return F.pad(t[None], (5, 5, 5, 5)) + (1 - inside) * pad_value.to(t.dtype)[None, :, None, None]

    xq = padded(xp)
    conv = lambda t: F.conv2d(t, window, groups=ch)[0]  # noqa: E731
    mu1, mu2 = conv(xq), conv(ypad)
    s1, s2, s12 = conv(xq * xq) - mu1 * mu1, conv(ypad * ypad) - mu2 * mu2, conv(xq * ypad) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s1 + s2 + R.C2))).mean()
    l1 = (xp - y).abs().mean()
    lam = R.lam32(lam)
    return dict(loss=(1 - lam) * l1 + lam * (1 - ssim), l1=l1, ssim=ssim)


def closed_forms(G, img, e):
    """(dL/dimg, dL/dexposure [C,2]) in float64 from G = dL/dx' (float64), the original image and e."""
    x, g = img.double(), e[:, 0].double()
    return g[:, None, None] * G, torch.stack(((G * x).sum((1, 2)), G.sum((1, 2))), dim=1)


def truth(img, gt, e, w1d, lam):
    """{xp, r64, r32, bar (loss_ref's, at (x', gt)), dimg, dexp (float64), bar_dimg, bar_dexp}."""
    xp = compensate(img, e)
    r64 = R.loss_parts(xp, gt, w1d, lam, torch.float64)
    r32 = R.loss_parts(xp, gt, w1d, lam, torch.float32)
    bar = R.bars(r64, r32, R.floors(xp, gt, w1d, lam))
    dimg, dexp = closed_forms(r64["grad"], img, e)
    bar_g, x, g = bar["grad"][1], img.double(), e[:, 0].double()
    bar_dimg = g.abs()[:, None, None] * bar_g + HALF * dimg.abs()
    bar_dexp = torch.stack(((bar_g * x.abs()).sum((1, 2)), bar_g.sum((1, 2))), dim=1) + HALF * dexp.abs()
    return dict(xp=xp, r64=r64, r32=r32, bar=bar, dimg=dimg, dexp=dexp, bar_dimg=bar_dimg, bar_dexp=bar_dexp)


def ratios(t, out3=None, dimg=None, dexp=None):
    """{name: largest |got - truth| / bar over ALL elements} for what is given; asserts that everything is finite."""
    res = {}
    if out3 is not None:
        got = dict(loss=float(out3[0]), l1=float(out3[1]), ssim=float(out3[2]))
        res.update({k: v[3] for k, v in R.worst_ratios(got, t["r64"], t["bar"]).items()})
    for name, got, want, bar in (("dimg", dimg, t["dimg"], t["bar_dimg"]), ("dexp", dexp, t["dexp"], t["bar_dexp"])):
        if got is not None:
            got = got.detach().double().cpu()
            assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
            err = (got - want).abs()
            res[name] = float(torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300)).max())
    return res


# ---- the shared cases ------------------------------------------------------------------------------------------------
def _cases():
    keys = ("rows", "rolled", "rolled2", "negative")
    out = []
    for i, s in enumerate(SHAPES):                 # every shape with every generator; lam and e rotate
        out += [(g, s, R.LAMS[(i + j) % 3], keys[(i + j) % 4]) for j, g in enumerate(GENS)]
    out += [("noise", (3, 33, 55), lam, k) for lam in R.LAMS for k in keys]   # every lam with every e across both seams
    out += [("edges", MANY, 0.2, "rows")]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


@functools.lru_cache(maxsize=4)
def _shared(key):
    name, shape, lam, ekey = key
    img, gt = R.make(name, shape)
    w, e = R.reference_window_1d(), exposure(ekey, shape[0])
    return dict(truth(img, gt, e, w, lam), img=img, gt=gt, e=e, w=w, lam=lam)


def case(name, shape, lam, ekey):
    """The cached truth is shared and never modified; the inputs a test may upload or change are copies."""
    c = _shared((name, tuple(shape), lam, ekey))
    return dict(c, img=c["img"].clone(), gt=c["gt"].clone(), e=c["e"].clone(), w=c["w"].clone())
