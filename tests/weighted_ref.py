"""Float64 truth, float32 yardstick and bars of the weighted photometric loss (csrc/weighted.hip), on the CPU.  Imports
loss_ref and exposure_ref and nothing from the package.

    x'(p) = fma(g_c, x(p), b_c) with an exposure (exposure_ref.compensate: the same float32 array on both sides), else x
    w(p)  = weights(p) * [acc(p) >= acc_min]          a NaN acc fails the comparison; [H,W], shared by the channels
    S     = sum_p w(p)
    l1    = sum_c sum_p w |x' - y| / (C S)            ssim = sum_c sum_q w(q) SSIM_c(q) / (C S)   (loss_ref's SSIM map:
    L     = (1 - lam) l1 + lam (1 - ssim)              grouped 11 x 11 conv2d over the FULL zero-padded x', y)
    mse_c = sum_p w (x' - y)^2 / S                     psnr = mean_c 20 log10(1 / sqrt(mse_c)), +inf where mse_c = 0
    S = 0:  L = l1 = ssim = mse = 0, psnr = +inf, every gradient zero
    G = dL/dx' from autograd;  dL/dimg = g_c G,  dL/dg_c = sum_p G x (the ORIGINAL x),  dL/db_c = sum_p G

`parts` evaluates this with the dtype as a parameter: float64 is the truth, float32 the yardstick e_ref = |f32 - f64|.
Every bar is max(2 e_ref, floor) per element, no element left out (for a gradient pixel e_ref is loss_ref.local_e_ref's
neighbourhood maximum).  The floors are loss_ref's counts plus the roundings the weights add, read from csrc/weighted.hip
before any kernel ran against them (a rounding is half a unit of 2^-23; K is in units):

  S        a thread adds its 8 weights, the wave's butterfly 6 levels, the four waves 2: 16 roundings on sum w (all
           terms >= 0); the per-unit float32 partials are added in float64 (nothing); out6[3] narrows once more
                                                                                   K_S = 8 (as a factor), K_SOUT = 9
  1/(C S)  formed in float64 and narrowed: the one rounding loss_ref already counts in "times float32(1 / N)"; but S's
           8 units reach EVERY normalised number as a relative error: + K_S on l1, ssim, mse and each gradient element
  l1       |d| 1, w |d| 1 (the product inside the fused multiply-add is not rounded; counted all the same), the sums
           16, times 1 / (C S) and the narrowing 2, S 16: 36 roundings                                    K_L1 = 18
  ssim     per pixel loss_ref's K_SSIM = 8 and `carried`, weighted by w; w n1 n2 one rounding, the sums 15, the two at
           the end 2, S 16: 34 roundings on sum w |SSIM| / (C S)                                         K_SUM = 17
  loss     loss_ref's K_MIX = 3 on (1 - lam) l1 + lam (1 + |ssim|)
  G        loss_ref's K_G = 26; the derivative maps are stored as w A, w B, w C: one rounding each; w sign(d) is exact;
           S 8 units                                                                         K_G = 26 + 1 + 8 = 35
           magnitude(p) = (1 - lam) / (C S) w(p) |sign| + lam / (C S) sum_q |k(p, q)| w(q) (magA + 2 |x'(p)| |B| + |y(p)| |C|)(q)
  mse_c    d 1 rounding, twice in d^2; w d 1; the fused add 1 per term: the sums 16; S 16; the float64 division and the
           narrowing 1: 36 roundings                                                                     K_MSE = 18
  psnr     = mean_c -10 log10(mse_c): an absolute 10 / ln(10) K_MSE 2^-23 and the narrowing's half unit of |psnr|; an
           infinite psnr (mse_c = 0) is compared for equality
  dL/dimg, dL/dexposure: exposure_ref's, from bar_G: |g| bar_G + 2^-24 |value|; sum bar_G |x| + 2^-24 |value|.

Weight patterns (`pattern`): see PATTERNS.  On shapes too small for a pattern's geometry the geometry is clipped so that
every pattern except `zero` keeps S > 0 (test_weighted_ref.py).  `mutant` evaluates eight wrong definitions in float64.
"""
import functools
import math

import torch
import torch.nn.functional as F

import exposure_ref as X
import loss_ref as R

E = R.EPS32
HALF = 2.0 ** -24
K = dict(S=8, S_out=9, l1=18, sum=17, ssim=R.K["ssim"], mix=R.K["mix"], grad=R.K["grad"] + 1 + 8, mse=18)
SHAPES = X.SHAPES
MANY = R.MANY_PARTIALS[0]
PATTERNS = ("ones", "frame", "blocks", "ramp", "corner", "seam", "zero", "gate")
EXPOSURES = (None, "rows", "negative")
ACC_MIN = 0.5
MUTANTS = ("norm_hw", "mask_images", "l1_grad_without_w", "maps_without_w", "gate_gt", "gate_lets_nan", "s_all_channels",
           "pad_with_bias")


# ---- weights -------------------------------------------------------------------------------------------------------
def _ramp(H, W):
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return (((7 * yy + 3 * xx + 4) % 11).float() / 10.0).contiguous()     # eleven levels in [0, 1], 0.4 at (0, 0)


def pattern(name, shape):
    """(weights [H,W] float32 or None, acc [H,W] float32 or None) of a named pattern on `shape`.
    ones    all one
    frame   a zero frame 12 pixels wide (the undistortion border), narrower where the image is: at least one pixel stays
    blocks  ones on blocks that straddle the work unit's seams x = 53 | 54 and y = 31 | 32 (each alone and both at once)
            and on the 2 x 2 corner; zero elsewhere
    ramp    eleven levels 0, 0.1 .. 1, non-binary
    corner  0.75 at (0, 0), zero elsewhere          seam    1 at the first pixel behind both seams (clipped to the image)
    zero    all zero
    gate    the ramp as weights and an acc image with values below (0.25), exactly at (0.5) and above (0.75, 1) acc_min
            = 0.5, and one NaN in the middle (where the image has more than one pixel)"""
    _, H, W = shape
    w = torch.zeros((H, W))
    if name == "ones":
        return torch.ones((H, W)), None
    if name == "frame":
        b = min(12, (min(H, W) - 1) // 2)
        w[b:H - b, b:W - b] = 1.0
        return w, None
    if name == "blocks":
        w[28:36, 10:20] = 1.0
        w[5:15, 50:58] = 1.0
        w[28:36, 50:58] = 1.0
        w[0:2, 0:2] = 1.0
        return w, None
    if name == "ramp":
        return _ramp(H, W), None
    if name == "corner":
        w[0, 0] = 0.75
        return w, None
    if name == "seam":
        w[min(32, H - 1), min(54, W - 1)] = 1.0
        return w, None
    if name == "zero":
        return w, None
    if name == "gate":
        yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
        acc = torch.tensor([0.25, 0.5, 0.75, 1.0])[(5 * yy + 2 * xx + 1) % 4].contiguous()
        if H * W > 1:
            acc[H // 2, W // 2] = float("nan")
        return _ramp(H, W), acc
    raise KeyError(name)


def effective(weights, acc, acc_min, shape, gate="ge"):
    """w = weights * [acc >= acc_min] as float32 [H,W].  gate: 'ge' (the definition), 'gt' and 'nan_passes' (mutants)."""
    _, H, W = shape
    w = torch.ones((H, W)) if weights is None else weights.float().clone()
    if acc is not None:
        a, m = acc.float(), torch.tensor(acc_min, dtype=torch.float32)
        keep = dict(ge=a >= m, gt=a > m, nan_passes=~(a < m))[gate]
        w = torch.where(keep, w, torch.zeros_like(w))
    return w


# ---- the restatement -----------------------------------------------------------------------------------------------
def ssim_map(x, y, w1d, separable=False, pad_value=None):
    """loss_ref.loss_parts' SSIM per pixel, [C,H,W] in x's dtype (differentiable in x).  separable: the kernels' order
    (two 11-tap passes, the variances through win(xx + yy)).  pad_value [C]: the MUTANT that pads x with it."""
    dtype, ch = x.dtype, x.shape[0]
    w = w1d.to(dtype)
    if pad_value is not None:
        inside = F.pad(torch.ones_like(x)[None], (5, 5, 5, 5))
        xq = F.pad(x[None], (5, 5, 5, 5)) + (1 - inside) * pad_value.to(dtype)[None, :, None, None]
        yq = F.pad(y[None], (5, 5, 5, 5))
        window = R._window(w, ch)
        conv = lambda t: F.conv2d(t, window, groups=ch)[0]  # noqa: E731
        mu1, mu2 = conv(xq), conv(yq)
        s1, s2, s12 = conv(xq * xq) - mu1 * mu1, conv(yq * yq) - mu2 * mu2, conv(xq * yq) - mu1 * mu2
        return ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s1 + s2 + R.C2))
    if separable:
        wv = w[None, None, :, None].expand(ch, 1, 11, 1).contiguous()
        wh = w[None, None, None, :].expand(ch, 1, 1, 11).contiguous()
        conv = lambda t: F.conv2d(F.conv2d(t[None], wv, padding=(5, 0), groups=ch), wh, padding=(0, 5), groups=ch)[0]  # noqa: E731
    else:
        window = R._window(w, ch)
        conv = lambda t: F.conv2d(t[None], window, padding=5, groups=ch)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s12 = conv(x * y) - mu1_mu2
    if separable:
        d2 = (conv(x * x + y * y) - mu1_sq - mu2_sq) + R.C2
    else:
        d2 = (conv(x * x) - mu1_sq) + (conv(y * y) - mu2_sq) + R.C2
    return ((2 * mu1_mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1_sq + mu2_sq + R.C1) * d2)


def _psnr(mse_c):
    return sum(math.inf if m == 0 else 20.0 * math.log10(1.0 / math.sqrt(m)) for m in mse_c) / len(mse_c)


def parts(xp, gt, w, w1d, lam, dtype, separable=False, norm=None, pad_value=None, drop_w_from_ssim_grad=False):
    """{loss, l1, ssim, S, mse, psnr (floats from `dtype`), mse_c (list), grad (float64 [C,H,W]: dL/dx')} of the
    definition at x' = xp.  norm: None = C S; a float = the MUTANT normaliser in its place.  drop_w_from_ssim_grad: the
    MUTANT whose SSIM gradient comes from the unweighted map (values unchanged)."""
    x = xp.detach().to(dtype).clone().requires_grad_(True)
    y, ww = gt.detach().to(dtype), w.to(dtype)
    ch = x.shape[0]
    S = ww.sum()
    if float(S) == 0.0:
        z = dict(loss=0.0, l1=0.0, ssim=0.0, S=0.0, mse=0.0, psnr=math.inf, mse_c=[0.0] * ch)
        return dict(z, grad=torch.zeros(x.shape, dtype=torch.float64))
    n = ch * S if norm is None else torch.tensor(norm, dtype=dtype)
    d = x - y
    sv = ssim_map(x, y, w1d, separable, pad_value)
    l1 = (ww * d.abs()).sum() / n
    ssim = (ww * sv).sum() / n
    lam = R.lam32(lam)
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    if drop_w_from_ssim_grad:
        grad = torch.autograd.grad((1 - lam) * l1 + lam * (1 - sv.sum() / n), x)[0].double()
    else:
        grad = torch.autograd.grad(loss, x)[0].double()
    s_one = n / ch if norm is not None else S
    mse_c = [float(v) for v in ((ww * d.detach() * d.detach()).sum((1, 2)) / s_one)]
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()), S=float(S),
                mse=sum(mse_c) / ch, psnr=_psnr(mse_c), mse_c=mse_c, grad=grad)


def parts_definition(xp, gt, w, w1d, lam):
    """The definition in float64 for TINY images by loops over pixels and taps (loss_ref.loss_parts_definition's window
    indexing), no convolution routine.  {loss, l1, ssim, S, mse, grad}."""
    x = xp.detach().double().clone().requires_grad_(True)
    y, ww, k = gt.detach().double(), w.double(), w1d.double()
    ch, H, W = x.shape
    S = float(ww.sum())
    tot_s, tot_l, tot_m = 0.0, 0.0, 0.0
    for c in range(ch):
        for qy in range(H):
            for qx in range(W):
                ys, xs, ws = [], [], []
                for ky in range(11):
                    for kx in range(11):
                        iy, ix = qy + ky - 5, qx + kx - 5
                        if 0 <= iy < H and 0 <= ix < W:
                            ys.append(iy), xs.append(ix), ws.append(float(k[ky]) * float(k[kx]))
                wv = torch.tensor(ws, dtype=torch.float64)
                a, b = x[c, ys, xs], y[c, ys, xs]
                mu1, mu2 = (wv * a).sum(), (wv * b).sum()
                s1, s2 = (wv * a * a).sum() - mu1 * mu1, (wv * b * b).sum() - mu2 * mu2
                s12 = (wv * a * b).sum() - mu1 * mu2
                sv = ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s1 + s2 + R.C2))
                wq = float(ww[qy, qx])
                tot_s = tot_s + wq * sv
                tot_l = tot_l + wq * (x[c, qy, qx] - y[c, qy, qx]).abs()
                tot_m = tot_m + wq * float((x[c, qy, qx] - y[c, qy, qx]).detach()) ** 2
    lam = R.lam32(lam)
    l1, ssim = tot_l / (ch * S), tot_s / (ch * S)
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()), S=S, mse=tot_m / (ch * S),
                grad=torch.autograd.grad(loss, x)[0])


# ---- the floors and the bars -----------------------------------------------------------------------------------------
def floors(xp, gt, w, w1d, lam):
    """loss_ref.floors with the weights (module docstring), float64: {l1, ssim, loss, S, mse, psnr (floats), grad}."""
    lam = R.lam32(lam)
    x, y, ww = xp.detach().double(), gt.detach().double(), w.double()
    ch = x.shape[0]
    S = float(ww.sum())
    n = ch * S
    k = w1d.double()
    window, wabs = R._window(k, ch), R._window(k.abs(), ch)
    conv = lambda t, kk=window: F.conv2d(t[None], kk, padding=5, groups=ch)[0]  # noqa: E731
    convT = lambda t, kk=window: F.conv_transpose2d(t[None], kk, padding=5, groups=ch)[0]  # noqa: E731
    leaf = lambda t: t.detach().clone().requires_grad_(True)  # noqa: E731
    mu1, mu2, es, e12 = leaf(conv(x)), leaf(conv(y)), leaf(conv(x * x + y * y)), leaf(conv(x * y))
    r_p1, r_p2, r_p12, r_s12, r_d2 = (leaf(torch.zeros_like(x)) for _ in range(5))
    p1, p2, p12 = mu1 * mu1 + r_p1, mu2 * mu2 + r_p2, mu1 * mu2 + r_p12
    s12 = e12 - p12 + r_s12
    n1, n2 = 2 * p12 + R.C1, 2 * s12 + R.C2
    d1, d2 = p1 + p2 + R.C1, (es - p1 + r_d2) - p2 + R.C2
    sv = n1 * n2 / (d1 * d2)
    ds_dmu1_t1, ds_dmu1_t2 = 2 * n2 * mu2 * d1 / (d1 * d1 * d2), -2 * n2 * mu1 * n1 / (d1 * d1 * d2)
    ds_ds1, ds_ds12 = -sv / d2, 2 * n1 / (d1 * d2)
    terms_a = (ds_dmu1_t1, ds_dmu1_t2, -2 * mu1 * ds_ds1, -mu2 * ds_ds12)
    A, B, Cm = sum(terms_a), ds_ds1, ds_ds12
    mag_a = sum(t.detach().abs() for t in terms_a)
    leaves = (mu1, mu2, es, e12, r_p1, r_p2, r_p12, r_s12, r_d2)
    errs = (R.K["mom1"] * E * conv(x.abs(), wabs), R.K["mom1"] * E * conv(y.abs(), wabs),
            R.K["mom2"] * E * conv(x * x + y * y, wabs), R.K["mom2"] * E * conv((x * y).abs(), wabs),
            0.5 * E * p1.detach(), 0.5 * E * p2.detach(), 0.5 * E * p12.detach().abs(), 0.5 * E * s12.detach().abs(),
            0.5 * E * (es - p1).detach().abs())

    def carried(f):
        gs = torch.autograd.grad(f.sum(), leaves, retain_graph=True, allow_unused=True)
        return sum(g.abs() * e for g, e in zip(gs, errs) if g is not None)

    c_sv, c_a, c_b, c_c = carried(sv), carried(A), carried(B), carried(Cm)
    sv, A, B, Cm = sv.detach(), A.detach(), B.detach(), Cm.detach()
    d = x - y
    l1 = float((ww * d.abs()).sum() / n)
    ssim = float((ww * sv).sum() / n)
    mse = float((ww * d * d).sum() / n)
    f_l1 = K["l1"] * E * l1
    f_ssim = float((ww * c_sv).sum() / n) + (K["ssim"] + K["sum"]) * E * float((ww * sv.abs()).sum() / n)
    f_loss = (1 - lam) * f_l1 + lam * f_ssim + K["mix"] * E * ((1 - lam) * l1 + lam * (1 + abs(ssim)))
    sgn = torch.sign(d)
    mag = (1 - lam) / n * ww * sgn.abs() + lam / n * (convT(ww * mag_a, wabs) + 2 * x.abs() * convT(ww * B.abs(), wabs)
                                                      + y.abs() * convT(ww * Cm.abs(), wabs))
    formula = (1 - lam) / n * ww * sgn - lam / n * (convT(ww * A) + 2 * x * convT(ww * B) + y * convT(ww * Cm))
    return dict(l1=f_l1, ssim=f_ssim, loss=f_loss, S=K["S_out"] * E * S, mse=K["mse"] * E * mse,
                psnr_abs=10.0 / math.log(10.0) * K["mse"] * E, grad=K["grad"] * E * mag, formula_grad=formula)


SCALARS = ("loss", "l1", "ssim", "S", "mse", "psnr")


def bars(r64, r32, fl):
    """{name: (e_ref, bar)}, bar = max(2 e_ref, floor); an infinite psnr has the bar 0 (equality)."""
    out = {}
    for k in ("loss", "l1", "ssim", "S", "mse"):
        e = abs(r32[k] - r64[k])
        out[k] = (e, max(2 * e, fl[k]))
    if math.isinf(r64["psnr"]):
        out["psnr"] = (0.0, 0.0)
    else:
        e = abs(r32["psnr"] - r64["psnr"]) if math.isfinite(r32["psnr"]) else 0.0
        out["psnr"] = (e, max(2 * e, fl["psnr_abs"] + 0.5 * E * abs(r64["psnr"])))
    e = R.local_e_ref((r32["grad"] - r64["grad"]).abs(), fl["grad"])
    out["grad"] = (e, torch.maximum(2 * e, fl["grad"]))
    return out


def closed_forms(G, img, e):
    """(dL/dimg, dL/dexposure or None) in float64 from G = dL/dx'."""
    if e is None:
        return G, None
    return X.closed_forms(G, img, e)


def truth(img, gt, e, weights, acc, acc_min, w1d, lam):
    """{xp, w, r64, r32, bar, dimg, dexp (float64; dexp None without an exposure), bar_dimg, bar_dexp}."""
    xp = img if e is None else X.compensate(img, e)
    w = effective(weights, acc, acc_min, img.shape)
    r64 = parts(xp, gt, w, w1d, lam, torch.float64)
    r32 = parts(xp, gt, w, w1d, lam, torch.float32)
    if r64["S"] == 0.0:
        zero = torch.zeros(img.shape, dtype=torch.float64)
        bar = {k: (0.0, 0.0) for k in SCALARS}
        bar["grad"] = (zero, zero)
        dexp = None if e is None else torch.zeros((img.shape[0], 2), dtype=torch.float64)
        return dict(xp=xp, w=w, r64=r64, r32=r32, bar=bar, dimg=zero, dexp=dexp, bar_dimg=zero,
                    bar_dexp=None if e is None else torch.zeros_like(dexp))
    bar = bars(r64, r32, floors(xp, gt, w, w1d, lam))
    dimg, dexp = closed_forms(r64["grad"], img, e)
    bar_g = bar["grad"][1]
    if e is None:
        return dict(xp=xp, w=w, r64=r64, r32=r32, bar=bar, dimg=dimg, dexp=None, bar_dimg=bar_g, bar_dexp=None)
    x, g = img.double(), e[:, 0].double()
    bar_dimg = g.abs()[:, None, None] * bar_g + HALF * dimg.abs()
    bar_dexp = torch.stack(((bar_g * x.abs()).sum((1, 2)), bar_g.sum((1, 2))), dim=1) + HALF * dexp.abs()
    return dict(xp=xp, w=w, r64=r64, r32=r32, bar=bar, dimg=dimg, dexp=dexp, bar_dimg=bar_dimg, bar_dexp=bar_dexp)


def ratios(t, out6=None, dimg=None, dexp=None):
    """{name: largest |got - truth| / bar over ALL elements} for what is given.  A zero bar asks for equality: ratio 0
    when equal, inf otherwise.  Asserts that every gradient element is finite."""
    res = {}
    if out6 is not None:
        got = [float(v) for v in out6]
        for i, k in enumerate(SCALARS):
            want, bar = t["r64"][k], t["bar"][k][1]
            if got[i] == want:
                res[k] = 0.0
            elif bar == 0.0 or not math.isfinite(got[i]) or not math.isfinite(want):
                res[k] = math.inf
            else:
                res[k] = abs(got[i] - want) / bar
    for name, got, want, bar in (("dimg", dimg, t["dimg"], t["bar_dimg"]), ("dexp", dexp, t["dexp"], t["bar_dexp"])):
        if got is not None:
            got = got.detach().double().cpu()
            assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
            err = (got - want).abs()
            r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300))
            res[name] = float(r.max())
    return res


# ---- mutants of the definition ---------------------------------------------------------------------------------------
def mutant(name, img, gt, e, weights, acc, acc_min, w1d, lam):
    """(out6 as a list, dimg, dexp) of a WRONG definition, float64 (the layout `ratios` takes):
    norm_hw            normalised by C H W instead of C S
    mask_images        the Torch-op route: plain loss of (w x', w y), rescaled by H W / S
    l1_grad_without_w  the L1 term of the gradient without w(p)
    maps_without_w     the derivative maps without w(q)
    gate_gt            acc > acc_min            gate_lets_nan   a NaN acc passes the gate
    s_all_channels     S summed over all C planes (C times too large)
    pad_with_bias      x' formed behind the padding: outside the image it is b_c"""
    ch, H, W = img.shape
    xp = img if e is None else X.compensate(img, e)
    gate = dict(gate_gt="gt", gate_lets_nan="nan_passes").get(name, "ge")
    w = effective(weights, acc, acc_min, img.shape, gate)
    kw = {}
    S = float(w.double().sum())
    if name == "norm_hw":
        kw = dict(norm=float(ch * H * W))
    elif name == "s_all_channels":
        kw = dict(norm=float(ch * ch * S))
    elif name == "pad_with_bias":
        kw = dict(pad_value=e[:, 1])
    elif name == "maps_without_w":
        kw = dict(drop_w_from_ssim_grad=True)
    if name == "mask_images":
        x = (xp.double() * w.double()).requires_grad_(True)
        r = X.loss64(x, gt.double() * w.double(), w1d, lam)
        scale = H * W / S
        G = torch.autograd.grad(r["loss"], x)[0] * w.double() * scale
        d = (xp.double() - gt.double()) * w.double()
        mse_c = [float(v) for v in (d * d).sum((1, 2)) / S]
        p = dict(loss=float(r["loss"].detach()) * scale, l1=float(r["l1"].detach()) * scale,
                 ssim=float(r["ssim"].detach()) * scale, S=S,
                 mse=sum(mse_c) / ch, psnr=_psnr(mse_c), grad=G)
    else:
        p = parts(xp, gt, w, w1d, lam, torch.float64, **kw)
    G = p["grad"]
    if name == "l1_grad_without_w":
        G = G + (1 - R.lam32(lam)) / (ch * S) * (1 - w.double()) * torch.sign(xp.double() - gt.double())
    dimg, dexp = closed_forms(G, img, e)
    return [p[k] for k in SCALARS], dimg, dexp


# ---- the shared cases ------------------------------------------------------------------------------------------------
def exposure(key, channels):
    return None if key is None else X.exposure(key, channels)


def _cases():
    out = []
    for i, s in enumerate(SHAPES):            # every shape x pattern x exposure; the generator and lam rotate
        for j, p in enumerate(PATTERNS):
            for k, ek in enumerate(EXPOSURES):
                out.append((X.GENS[(i + j + k) % 4], s, R.LAMS[(i + j + 2 * k) % 3], p, ek))
    out.append(("edges", MANY, 0.2, "ramp", "rows"))     # > 1024 partials per channel, once
    return out


CASES = _cases()


@functools.lru_cache(maxsize=4)
def _shared(key):
    name, shape, lam, pat, ekey = key
    img, gt = R.make(name, shape)
    w1d, e = R.reference_window_1d(), exposure(ekey, shape[0])
    weights, acc = pattern(pat, shape)
    return dict(truth(img, gt, e, weights, acc, ACC_MIN, w1d, lam), img=img, gt=gt, e=e, weights=weights, acc=acc,
                win=w1d, lam=lam)


def case(name, shape, lam, pat, ekey):
    """The cached truth is shared and never modified; the inputs a test may upload or change are copies."""
    c = _shared((name, tuple(shape), lam, pat, ekey))
    cl = lambda t: None if t is None else t.clone()  # noqa: E731
    return dict(c, img=c["img"].clone(), gt=c["gt"].clone(), e=cl(c["e"]), weights=cl(c["weights"]), acc=cl(c["acc"]),
                win=c["win"].clone())
