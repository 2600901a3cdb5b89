"""Plain-Torch restatement of the photometric loss (csrc/loss.hip) with the dtype as a parameter, on the CPU, the bars
the kernels are held to, and the inputs they are held on.  Nothing here imports the package.

    L = (1 - lam) * mean|x - y| + lam * (1 - mean(SSIM(x, y)))        x = img, y = gt, [C][H][W]
    SSIM(q) = (2 mu1 mu2 + C1) (2 s12 + C2) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2))
    mu1 = win(x), mu2 = win(y), s1 = win(x x) - mu1^2, s2 = win(y y) - mu2^2, s12 = win(x y) - mu1 mu2
    win(f)(q) = sum_k w[ky] w[kx] f(q + k - 5), zero outside the image          (cross-correlation, NOT convolution)

`loss_parts` builds this as the reference does (grouped 11 x 11 conv2d, padding 5, five moments) and takes dL/dimg from
autograd.  `loss_parts_definition` evaluates the same definition for tiny images by a loop over pixels and taps with
explicit index arithmetic -- no convolution routine, so the orientation of the (asymmetric) window and the zero padding
are not anchored on conv2d's conventions.  lam is narrowed to float32 first (the C ABI takes a float) and C1 / C2 are the
doubles 1e-4 / 9e-4 (the reference and the kernel round them to float32: one rounding, counted below).

Run in float64 the restatement is the truth; run in float32 it is the yardstick e_ref = |float32 - float64|.  The bar of
every compared number is, per element and with no element left out,

    max(2 e_ref, floor),     floor = K 2^-23 magnitude     (the three scalars: + carried, below)

in the style of optim_ref.py.  A rounding is half a unit (2^-24 relative); K is in units of 2^-23 = two roundings.

Windowed moments (the kernel: vertical 11-tap pass, then horizontal 11-tap pass, each a plain running sum).  The first
term of an 11-tap running sum is rounded by its product and by 10 additions: 11 roundings a pass, 22 for both: 11 units of
win|f|.  The products x x + y y (a multiply and a fused multiply-add) and x y add 2 and 1 roundings: 12 units.
    err(mu1) = 11 E win|x|, err(mu2) = 11 E win|y|, err(win(xx + yy)) = 12 E win(xx + yy), err(win(xy)) = 12 E win|xy|

`carried`: SSIM's algebra cancels -- s12 = win(xy) - mu1 mu2, d2 = win(xx + yy) - mu1^2 - mu2^2 + C2, and where the planes
are flat only C2 = 9e-4 is left of d2, so the roundings above reach SSIM amplified by win(xx + yy) / C2.  That is a
property of the formula in float32, the reference's evaluation included (test_gpu_loss.py: variance_rounding_slack).  It
is propagated to first order, in float64, through SSIM written as a function of nine independent leaves: the four moments
with the errors above, and the five intermediates that are subtracted from something of their own size, half a unit of
2^-23 each: mu1^2, mu2^2, mu1 mu2, s12 and win(xx + yy) - mu1^2.  carried(F) = sum_leaf |dF / dleaf| err(leaf), the
derivatives from autograd.  The same propagation is applied to the three maps the backward filters,
    A = dSSIM/dmu1 (total: through mu1^2 and mu1 mu2), B = dSSIM/ds1, C = dSSIM/ds12.

What is left after the leaves does not cancel and is counted in K (roundings, i.e. half units):
  SSIM     n1, n2, d1, d2: an add and the rounded constant, 2 each = 8; two hardware reciprocals good to 1 ulp = 2
           roundings each = 4; their product 1; n1 * n2 * inv 2: 15 roundings                               K_SSIM = 8
  A        its longest chain is -2 mu1 * (-SSIM / d2): SSIM 15, reciprocal 2, multiply 1, times 2 mu1 1, subtract 1: 20
           roundings; the difference mu2 d1 - mu1 n1 inside dSSIM/dmu1 cancels where img ~ gt, so the magnitude of A is
           the sum of the absolute values of its terms (`magA`), not |A|                                     K_ABC = 10
  sums     a thread adds at most 8 (L1) or 7 (SSIM) values, a wave's butterfly 6 levels, the four waves 2: 16 / 15
           roundings on sum|term|; the partials are added in float64 (nothing); times float32(1 / N) and the narrowing
           to float32: 2 more.  |x - y| itself: 1.                       K_L1 = (1 + 16 + 2) / 2 -> 10, K_SUM = (15 + 2) / 2 -> 9
  loss     1 - lam, 1 - ssim (an ABSOLUTE half unit of 1), two multiplies, an add: 5 roundings on
           (1 - lam) l1 + lam (1 + |ssim|)                                                                   K_MIX = 3
  dL/dimg  = (1 - lam) / N sign(x - y) - lam / N [winT(A) + 2 x winT(B) + y winT(C)],  winT the transposed window:
           two 11-tap passes 11 units; A, B, C's own K_ABC = 10; 2 x *, y *, two adds, lam / N (rounded 1 / N, a
           multiply), the multiply and the subtraction: 9 roundings -> 5 units                                 K_G = 26
           magnitude(p) = (1 - lam) / N |sign| + lam / N sum_q |w(p, q)| (magA(q) + 2 |x(p)| |B(q)| + |y(p)| |C(q)|)
           The gradient floor has NO carried term.  Where the planes are flat the cancellation above does reach the
           gradient, and there the bar is what the reference's own float32 error says it is: e_ref.  One pixel's
           |e_ref| is a single draw of that error and may be near zero by accident, so for a gradient pixel
               e_ref(p) = floor(p) * max over the 21 x 21 pixels q of the plane around p of |float32 - float64|(q) / floor(q)
           -- how far float32 leaves the counted floor is a property of the region (the roundings that reach p were made
           in the windows within 5 pixels of it, which see the image within 10 pixels; the neighbours' errors are draws
           from the same windows), while the floor itself follows the pixel (|x(p)|, |y(p)|).  So
               bar(p) = K_G E magnitude(p) * max(1, 2 max_q e(q) / floor(q))
           Measured on the CPU at (3, 33, 55), lam = 1, the factor max(1, .), median / largest over the pixels:
           noise, dark, bright, equal_but_one 1 / 1 (the bar IS the issue's), ramp 1 / 1, edges 1.03 / 3.9.  A worst-case
           propagation of `carried` into the gradient would be 11 ... 1100 times the floor; it is only reported
           (`grad_worst_case`).

The scalar floors (one accidental near-zero e_ref must not define the bar of a single number):
  l1    K_L1 E l1
  ssim  mean(carried SSIM) + (K_SSIM + K_SUM) E mean|SSIM|
  loss  (1 - lam) floor(l1) + lam floor(ssim) + K_MIX E ((1 - lam) l1 + lam (1 + |ssim|))

The counts were fixed from csrc/loss.hip before any kernel ran against them; what the kernels measure is in DESIGN.md.

Inputs (all seeded, float32, CPU): see GENERATORS.  `bright` stops at 4.  The float32 restatement was walked up in
amplitude on the CPU (test_loss_ref.py repeats the walk): on noise and edges its three scalars stay inside the floors
alone (no 2 e_ref) at every amplitude tried, up to 256; on constant planes a against 0.75 a, where d2 is C2 = 9e-4 plus the rounding
of win(xx + yy) - mu1^2 - mu2^2 (~ 1.6 a^2 each), its smallest d2 is 8.9e-4 at a = 4, 3.5e-4 at a = 32 and NEGATIVE at
a = 48.  So 32 is the last amplitude at which the reference's own float32 formula is meaningful on flat regions; 4 -- what
an unclamped render with SH colour produces -- is a factor 8 inside.

The float32 restatement against K_G E magnitude alone (CPU, (3, 33, 55), lam = 1): noise 0.14, ramp 0.36, edges 1.9 --
on flat blocks the reference leaves the count-only floor, which is why max(2 e_ref, .) is there.  test_loss_ref.py holds
a second float32 evaluation (`separable=True`: two 11-tap passes, four moments, the kernel's order of operations in
Torch) inside every bar on every case, so the bars are not vacuous for the evaluation they were taken from.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 * 0.01, 0.03 * 0.03
EPS32 = 2.0 ** -23
K = dict(mom1=11, mom2=12, ssim=8, abc=10, l1=10, sum=9, mix=3, grad=26)
REACH = 21   # pixels: a gradient pixel depends on the image within 10 pixels of it (two 11-tap windows)
BRIGHT_AMPLITUDE = 4.0
LAMS = (0.0, 0.2, 1.0)


def reference_window_1d():
    """The reference's 1-D window (its exponent floors (x - 11) / 2: NOT the centred Gaussian), float32, written from
    the formula so that this module does not import the package; test_loss_ref.py holds it equal to the package's."""
    g = [math.exp(-(math.floor((x - 11) / 2.0) ** 2) / (2.0 * 1.5 * 1.5)) for x in range(11)]
    t = torch.tensor(g, dtype=torch.float32)
    return t / t.sum()


def symmetric_window_1d():
    x = torch.arange(11, dtype=torch.float32) - 5
    w = torch.exp(-x * x / 4.5)
    return w / w.sum()


def lam32(lam):
    return float(np.float32(lam))


def _window(w, ch):
    return (w[:, None] @ w[None, :])[None, None].expand(ch, 1, 11, 11).contiguous()


# ---- the restatement -----------------------------------------------------------------------------------------------
def loss_parts(img, gt, w1d, lam, dtype, want_grad=True, separable=False):
    """{loss, l1, ssim (python floats, from `dtype`), grad (float64 tensor: d loss / d img through autograd), d2_min}.
    separable=True: the same function in ANOTHER order of operations -- an 11 x 1 pass, then a 1 x 11 pass, and the two
    variances through their sum win(xx + yy) -- used in float32 on the CPU to show that the bars hold for a float32
    evaluation that is not the one e_ref was taken from (test_loss_ref.py)."""
    x = img.detach().to(dtype).clone().requires_grad_(want_grad)
    y = gt.detach().to(dtype)
    ch = x.shape[0]
    window = _window(w1d.to(dtype), ch)
    conv = lambda t: F.conv2d(t[None], window, padding=5, groups=ch)[0]  # noqa: E731
    if separable:
        wv = w1d.to(dtype)[None, None, :, None].expand(ch, 1, 11, 1).contiguous()
        wh = w1d.to(dtype)[None, None, None, :].expand(ch, 1, 1, 11).contiguous()
        conv = lambda t: F.conv2d(F.conv2d(t[None], wv, padding=(5, 0), groups=ch), wh, padding=(0, 5), groups=ch)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s12 = conv(x * y) - mu1_mu2
    if separable:
        d2 = (conv(x * x + y * y) - mu1_sq - mu2_sq) + C2
    else:
        s1 = conv(x * x) - mu1_sq
        s2 = conv(y * y) - mu2_sq
        d2 = s1 + s2 + C2
    ssim = (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * d2)).mean()
    l1 = (x - y).abs().mean()
    lam = lam32(lam)
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    out = dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()),
               d2_min=float(d2.detach().min()))
    if want_grad:
        out["grad"] = torch.autograd.grad(loss, x)[0].double()
    return out


def loss_parts_definition(img, gt, w1d, lam):
    """The definition in float64 for TINY images: a loop over output pixels and over the 11 x 11 taps, the input pixel of
    tap (ky, kx) at output (qy, qx) being (qy + ky - 5, qx + kx - 5), skipped (zero) outside the image."""
    x = img.detach().double().clone().requires_grad_(True)
    y = gt.detach().double()
    w = w1d.double()
    ch, H, W = x.shape
    total, count = 0.0, 0
    for c in range(ch):
        for qy in range(H):
            for qx in range(W):
                ys, xs, ws = [], [], []
                for ky in range(11):
                    for kx in range(11):
                        iy, ix = qy + ky - 5, qx + kx - 5
                        if 0 <= iy < H and 0 <= ix < W:
                            ys.append(iy)
                            xs.append(ix)
                            ws.append(float(w[ky]) * float(w[kx]))
                wv = torch.tensor(ws, dtype=torch.float64)
                a, b = x[c, ys, xs], y[c, ys, xs]
                mu1, mu2 = (wv * a).sum(), (wv * b).sum()
                s1 = (wv * a * a).sum() - mu1 * mu1
                s2 = (wv * b * b).sum() - mu2 * mu2
                s12 = (wv * a * b).sum() - mu1 * mu2
                total = total + ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
                count += 1
    ssim = total / count
    l1 = (x - y).abs().sum() / count
    lam = lam32(lam)
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()),
                grad=torch.autograd.grad(loss, x)[0])


def impulse_ssim_gradient(shape, py, px, amp, w1d):
    """d mean(SSIM) / d img for img = amp at (py, px) of every channel and zero elsewhere, gt = 0, in closed form.
    With W(q, p) = w[py - qy + 5] w[px - qx + 5] the weight of pixel p in the window of output q (zero unless both
    indices lie in 0..10):  mu1(q) = amp W(q, p0),  win(xx)(q) = amp^2 W(q, p0),  mu2 = s2 = s12 = 0, so
        SSIM(q) = C1 C2 / (d1 d2),   d1 = mu1^2 + C1,   d2 = win(xx) - mu1^2 + C2
        dSSIM/dmu1 = 2 mu1 SSIM (1 / d2 - 1 / d1)   (at fixed win(xx)),     dSSIM/dwin(xx) = -SSIM / d2
        d mean / d x(p) = 1 / N sum_q W(q, p) (dSSIM/dmu1(q) + 2 x(p) dSSIM/dwin(xx)(q))
    Plain loops over q and p; float64; the same for every channel."""
    ch, H, W = shape
    w = [float(v) for v in w1d.double()]
    tap = lambda q, p: w[p - q + 5] if 0 <= p - q + 5 <= 10 else 0.0  # noqa: E731
    N = ch * H * W
    dmu, de = {}, {}
    for qy in range(max(0, py - 5), min(H, py + 6)):
        for qx in range(max(0, px - 5), min(W, px + 6)):
            wq = tap(qy, py) * tap(qx, px)
            mu1, e11 = amp * wq, amp * amp * wq
            d1, d2 = mu1 * mu1 + C1, e11 - mu1 * mu1 + C2
            s = C1 * C2 / (d1 * d2)
            dmu[qy, qx] = 2 * mu1 * s * (1 / d2 - 1 / d1)
            de[qy, qx] = -s / d2
    g = torch.zeros((H, W), dtype=torch.float64)
    for y in range(max(0, py - 10), min(H, py + 11)):
        for x in range(max(0, px - 10), min(W, px + 11)):
            v = amp if (y, x) == (py, px) else 0.0
            acc = 0.0
            for (qy, qx), a in dmu.items():
                acc += tap(qy, y) * tap(qx, x) * (a + 2 * v * de[qy, qx])
            g[y, x] = acc / N
    return g[None].expand(ch, H, W)


# ---- the floors ----------------------------------------------------------------------------------------------------
def floors(img, gt, w1d, lam):
    """{l1, ssim, loss (floats), grad (tensor)}: the K 2^-23 magnitude + carried part of every bar (module docstring),
    in float64.  Also 'formula_grad': dL/dimg assembled from A, B, C as written here (held to autograd on the CPU, so that
    the maps the floors are made from are the right ones)."""
    E = EPS32
    lam = lam32(lam)
    x, y = img.detach().double(), gt.detach().double()
    ch = x.shape[0]
    N = x.numel()
    w = w1d.double()
    window, wabs = _window(w, ch), _window(w.abs(), ch)
    conv = lambda t, k=window: F.conv2d(t[None], k, padding=5, groups=ch)[0]  # noqa: E731
    convT = lambda t, k=window: F.conv_transpose2d(t[None], k, padding=5, groups=ch)[0]  # noqa: E731
    leaf = lambda t: t.detach().clone().requires_grad_(True)  # noqa: E731
    mu1, mu2, es, e12 = leaf(conv(x)), leaf(conv(y)), leaf(conv(x * x + y * y)), leaf(conv(x * y))
    r_p1, r_p2, r_p12, r_s12, r_d2 = (leaf(torch.zeros_like(x)) for _ in range(5))
    p1, p2, p12 = mu1 * mu1 + r_p1, mu2 * mu2 + r_p2, mu1 * mu2 + r_p12
    s12 = e12 - p12 + r_s12
    n1, n2 = 2 * p12 + C1, 2 * s12 + C2
    d1, d2 = p1 + p2 + C1, (es - p1 + r_d2) - p2 + C2
    sv = n1 * n2 / (d1 * d2)
    # the chain rule at fixed gt: through mu1, s1 = win(xx) - mu1^2, s12 = win(xy) - mu1 mu2
    ds_dmu1_t1, ds_dmu1_t2 = 2 * n2 * mu2 * d1 / (d1 * d1 * d2), -2 * n2 * mu1 * n1 / (d1 * d1 * d2)
    ds_ds1 = -sv / d2
    ds_ds12 = 2 * n1 / (d1 * d2)
    terms_a = (ds_dmu1_t1, ds_dmu1_t2, -2 * mu1 * ds_ds1, -mu2 * ds_ds12)
    A, B, Cm = sum(terms_a), ds_ds1, ds_ds12
    mag_a = sum(t.detach().abs() for t in terms_a)
    leaves = (mu1, mu2, es, e12, r_p1, r_p2, r_p12, r_s12, r_d2)
    errs = (K["mom1"] * E * conv(x.abs(), wabs), K["mom1"] * E * conv(y.abs(), wabs),
            K["mom2"] * E * conv(x * x + y * y, wabs), K["mom2"] * E * conv((x * y).abs(), wabs),
            0.5 * E * p1.detach(), 0.5 * E * p2.detach(), 0.5 * E * p12.detach().abs(), 0.5 * E * s12.detach().abs(),
            0.5 * E * (es - p1).detach().abs())

    def carried(f):
        gs = torch.autograd.grad(f.sum(), leaves, retain_graph=True, allow_unused=True)
        return sum(g.abs() * e for g, e in zip(gs, errs) if g is not None)

    c_sv, c_a, c_b, c_c = carried(sv), carried(A), carried(B), carried(Cm)
    sv, A, B, Cm = sv.detach(), A.detach(), B.detach(), Cm.detach()
    l1 = float((x - y).abs().mean())
    ssim = float(sv.mean())
    f_l1 = K["l1"] * E * l1
    f_ssim = float(c_sv.mean()) + (K["ssim"] + K["sum"]) * E * float(sv.abs().mean())
    f_loss = (1 - lam) * f_l1 + lam * f_ssim + K["mix"] * E * ((1 - lam) * l1 + lam * (1 + abs(ssim)))
    sgn = torch.sign(x - y)
    mag = (1 - lam) / N * sgn.abs() + lam / N * (convT(mag_a, wabs) + 2 * x.abs() * convT(B.abs(), wabs)
                                                 + y.abs() * convT(Cm.abs(), wabs))
    car = lam / N * (convT(c_a, wabs) + 2 * x.abs() * convT(c_b, wabs) + y.abs() * convT(c_c, wabs))
    formula = (1 - lam) / N * sgn - lam / N * (convT(A) + 2 * x * convT(B) + y * convT(Cm))
    return dict(l1=f_l1, ssim=f_ssim, loss=f_loss, grad=K["grad"] * E * mag, grad_worst_case=K["grad"] * E * mag + car,
                formula_grad=formula,
                d2_min=float(d2.detach().min()))


def local_e_ref(e, floor):
    """e_ref of a gradient pixel (module docstring: dL/dimg): floor(p) times the largest e / floor among the
    REACH x REACH pixels of the plane around p."""
    rel = torch.where(floor > 0, e / floor.clamp(min=1e-300), torch.zeros_like(e))
    return floor * F.max_pool2d(rel[None], REACH, stride=1, padding=REACH // 2)[0]


def bars(r64, r32, fl):
    """{name: (e_ref, bar)}: e_ref = |float32 restatement - float64| (for 'grad': its maximum over the pixel's
    neighbourhood, `local_e_ref`), bar = max(2 e_ref, floor); floats for the three scalars, tensors for 'grad'."""
    out = {}
    for k in ("loss", "l1", "ssim"):
        e = abs(r32[k] - r64[k])
        out[k] = (e, max(2 * e, fl[k]))
    e = local_e_ref((r32["grad"] - r64["grad"]).abs(), fl["grad"])
    out["grad"] = (e, torch.maximum(2 * e, fl["grad"]))
    return out


def worst_ratios(got, r64, bar):
    """{name: (err, e_ref, bar, err / bar)}; for 'grad' the maxima over ALL pixels, the ratio taken per pixel first.
    got: {loss, l1, ssim: float, grad: tensor} (any subset)."""
    res = {}
    for k in ("loss", "l1", "ssim"):
        if k in got:
            err = abs(float(got[k]) - r64[k])
            assert math.isfinite(err), (k, got[k])
            res[k] = (err, bar[k][0], bar[k][1], err / bar[k][1] if err else 0.0)
    if got.get("grad") is not None:
        g = got["grad"].double().cpu()
        assert bool(torch.isfinite(g).all()), "non-finite gradient"
        err = (g - r64["grad"]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bar["grad"][1].clamp(min=1e-300))
        res["grad"] = (float(err.max()), float(bar["grad"][0].max()), float(bar["grad"][1].max()), float(ratio.max()))
    return res


# ---- inputs --------------------------------------------------------------------------------------------------------
def _gen(shape, seed):
    return torch.Generator().manual_seed(7919 * seed + 31 * shape[1] + shape[2] + 1000003 * shape[0])


def noise(shape, seed=0, amplitude=1.0):
    """test_gpu_loss.py's: uniform noise against 0.6 noise + 0.4 of the image rolled by one column."""
    g = _gen(shape, seed)
    img = torch.rand(shape, generator=g)
    gt = (0.6 * torch.rand(shape, generator=g) + 0.4 * img.roll(1, 2)).clamp(0, 1)
    return img * amplitude, gt * amplitude


def dark(shape, seed=0):
    """values <= 0.02: mu^2 <= 4e-4 and the sigmas <= 4e-4, so C1 = 1e-4 and C2 = 9e-4 carry both denominators."""
    return noise(shape, seed + 1, 0.02)


def bright(shape, seed=0):
    """values up to BRIGHT_AMPLITUDE = 4 (a render is not clamped above; the cap is derived in the module docstring)."""
    return noise(shape, seed + 2, BRIGHT_AMPLITUDE)


def edges(shape, seed=0, amplitude=1.0):
    """Piecewise-constant 7 x 13 blocks (neither divides 32 x 54) with one-pixel transitions; the target's block grid is
    shifted by (3, 5) and a third of its blocks repeat the image's level, so flat-on-flat, edge-on-flat and equal
    regions all occur."""
    g = _gen(shape, seed + 3)
    ch, H, W = shape
    nby, nbx = H // 7 + 2, W // 13 + 2
    la = torch.rand((ch, nby, nbx), generator=g)
    lb = torch.where(torch.rand((ch, nby, nbx), generator=g) < 1 / 3, la, torch.rand((ch, nby, nbx), generator=g))
    yy, xx = torch.arange(H), torch.arange(W)
    img = la[:, (yy // 7)[:, None], (xx // 13)[None, :]]
    gt = lb[:, ((yy + 3) // 7)[:, None], ((xx + 5) // 13)[None, :]]
    return (img * amplitude).contiguous(), (gt * amplitude).contiguous()


def ramp(shape, seed=0):
    """Smooth gradients: a plane per channel for the image, another for the target."""
    g = _gen(shape, seed + 4)
    ch, H, W = shape
    c = torch.rand((6, ch, 1, 1), generator=g)
    v = torch.linspace(0, 1, H)[None, :, None]
    u = torch.linspace(0, 1, W)[None, None, :]
    img = 0.1 + 0.5 * c[0] * u + 0.4 * c[1] * v + 0.0 * c[2]
    gt = 0.05 + 0.45 * c[3] * u + 0.5 * c[4] * (1 - v) + 0.0 * c[5]
    return img.expand(shape).contiguous().float(), gt.expand(shape).contiguous().float()


def one_pixel(shape):
    """The pixel equal_but_one moves: last channel, middle row, middle column."""
    return shape[0] - 1, shape[1] // 2, shape[2] // 2


def equal_but_one(shape, seed=0):
    g = _gen(shape, seed + 5)
    gt = torch.rand(shape, generator=g)
    img = gt.clone()
    c, y, x = one_pixel(shape)
    img[c, y, x] = gt[c, y, x] + 0.25
    return img, gt


def impulse(shape, y, x, target=0.0, amplitude=1.0):
    """One nonzero pixel (every channel) in a zero image against a constant target (0 or e.g. 0.5)."""
    img = torch.zeros(shape)
    img[:, y, x] = amplitude
    return img, torch.full(shape, float(target))


GENERATORS = dict(noise=noise, dark=dark, bright=bright, edges=edges, ramp=ramp, equal_but_one=equal_but_one)

# ---- the cases of test_gpu_loss_ref64.py (here, so that test_loss_ref.py can hold the float32 restatement on them) ---
# the smallest shapes at which each mechanism engages: H or W in {1, 2, 5, 6, 10, 11, 12} (the halo), W in {53, 54, 55,
# 59, 60, 107, 108, 109} and H in {31, 32, 33, 37, 38, 63, 64, 65} (the 54 x 32 work unit and work unit + halo), C in
# {1, 3, 4}; the last three cross a seam on both axes at once
SEAM_SHAPES = [(1, 1, 1), (3, 1, 53), (1, 2, 54), (3, 5, 55), (4, 6, 59), (3, 10, 60), (1, 11, 107), (3, 12, 108),
               (3, 31, 109), (3, 32, 1), (1, 33, 2), (3, 37, 5), (4, 38, 6), (3, 63, 10), (1, 64, 11), (3, 65, 12),
               (3, 33, 55), (1, 65, 109), (4, 38, 60)]
# 1026 work units (> the 1024 threads of k_loss_finalize) from few pixels
MANY_PARTIALS = [(3, 1, 54 * 342), (3, 32 * 342, 1)]
BOTH_SEAMS = [(3, 33, 55), (1, 65, 109), (4, 38, 60)]
_NAMES = tuple(GENERATORS)


def _cases():
    out = []
    for i, s in enumerate(SEAM_SHAPES):          # every seam shape with two generators (rotating) and lam = 0.2 ...
        out += [(_NAMES[i % 6], s, 0.2), (_NAMES[(i + 3) % 6], s, LAMS[(i + 2) % 3])]
    for s in BOTH_SEAMS:                         # ... and every generator at every lam where both axes cross a seam
        out += [(g, s, lam) for g in _NAMES for lam in LAMS]
    out += [("noise", MANY_PARTIALS[0], 0.2), ("edges", MANY_PARTIALS[1], 1.0)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


def impulse_cases():
    """(shape, y, x, target, lam): corners, each border, and both sides of x = 53 | 54 and y = 31 | 32."""
    s = (3, 38, 60)
    H, W = s[1], s[2]
    at = [(0, 0), (H - 1, W - 1), (0, 30), (H - 1, 30), (17, 0), (17, W - 1), (17, 53), (17, 54), (31, 20), (32, 20),
          (31, 53), (32, 54)]
    out = [(s, y, x, (0.0, 0.5)[i % 2], (1.0, 0.2)[(i // 2) % 2]) for i, (y, x) in enumerate(at)]
    return out + [((1, 1, 1), 0, 0, 0.0, 1.0), ((1, 2, 12), 1, 11, 0.5, 1.0)]


def make(name, shape):
    return GENERATORS[name](shape)


@functools.lru_cache(maxsize=4)
def _shared(key):
    """float64 restatement and floors of one (inputs, lam): computed once, shared, never modified."""
    kind, args, lam = key
    img, gt = impulse(*args) if kind == "impulse" else make(kind, args)
    w = reference_window_1d()
    r64 = loss_parts(img, gt, w, lam, torch.float64)
    r32 = loss_parts(img, gt, w, lam, torch.float32)
    fl = floors(img, gt, w, lam)
    return dict(img=img, gt=gt, w=w, lam=lam, r64=r64, r32=r32, floors=fl, bar=bars(r64, r32, fl))


def _handout(c):
    """The cached reference is shared; the inputs a test may upload or modify are copies."""
    return dict(c, img=c["img"].clone(), gt=c["gt"].clone(), w=c["w"].clone())


def case(name, shape, lam):
    return _handout(_shared((name, tuple(shape), lam)))


def impulse_case(shape, y, x, target, lam):
    return _handout(_shared(("impulse", (tuple(shape), y, x, target), lam)))
