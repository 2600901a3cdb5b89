"""Robust LiDAR depth supervision (csrc/lidar.hip: gsr_lidar_occlusion_filter, gsr_lidar_depth_loss_robust) restated
for the tests.

filter32()    the occlusion filter: a loop over the pixels, each with its clamped window, the removal test in numpy
              float32 scalars -- one subtraction, one product, one compare.  Every operation is exact IEEE (a minimum
              selects, the three float32 operations round as the kernel's), so this IS the contract: every test of the
              filter is an equality.
filter_ops()  the same in Torch ops, -max_pool2d(-where(z > 0, z, inf)) with its implicit padding of -inf (+inf for
              the minimum): what a caller composes without the fused call (tools/time_lidar_robust.py times it);
              tests/test_lidar_robust_ref.py holds it equal to filter32.
robust_ops()  the Huber / clip depth loss in plain Torch with the gradients from autograd; float64 is the truth,
              float32 the yardstick.  At the identity parameters (huber 0, clip +inf) it is lidar_ref.loss_ops exactly.
bars()        the bound of the fused call's error against float64 per compared quantity, and the fragile sets.
inputs() / reference() / exact_case()   the inputs of tests/test_gpu_lidar_robust.py and their references, evaluated
              once per process and not to be modified.

Bars.  eps = 2^-23 per counted rounding, as tests/lidar_ref.py counts; the four parameters are float32 values on both
sides (HUBER_ABS = float32(0.1), ...), so they carry no rounding.  Per candidate pixel (z_L > 0 and A >= acc_min):
  e = D / A - z_L                  one division, one subtraction                  de = eps (|D / A| + |e|)   (lidar_ref)
  a = |e|                          exact                                          da = de
  tau = h_abs + h_rel z_L          one fma or a product and a sum                 dtau = 2 eps tau
  clip = c_abs + c_rel z_L         likewise                                       dclip = 2 eps clip
  quadratic zone, a < tau:
    rho = 0.5 a (a / tau)          a / tau, one product (0.5 a is exact)          drho = |psi| de + 0.5 psi^2 dtau + 2 eps rho
    psi = e / tau                  one division                                   dpsi = de / tau + dtau / tau + eps |psi|
        (d rho / da = a / tau = |psi|, d rho / dtau = -0.5 psi^2; |psi| <= 1 bounds the dtau term of psi)
  linear zone:
    rho = a - 0.5 tau              one subtraction (or one fma: 0.5 tau is exact)  drho = de + 0.5 dtau + eps rho
    psi = sign(e)                  exact                                          dpsi = 0
  a pixel within de + dtau of tau may be evaluated on the other branch.  rho is C1 there: the two formulas differ by
  0.5 (a - tau)^2 / tau, second order, far inside eps rho.  psi is continuous but not C1: the formulas differ by
  |a - tau| / tau <= (de + dtau) / tau, which the quadratic zone's dpsi covers; a LINEAR pixel within de + dtau of tau
  gets the quadratic dpsi too.  So there is no fragile set for tau.
  sum rho / n_sup: f64 partial sums, one division, one narrowing                  dmean_rho = sum drho / n_sup + 3 eps mean_rho
  L = lambda mean_rho              one product                                    dL = |lambda| dmean_rho + eps |L|
  mean a: as lidar_ref's mean                                                     dmean = sum de / n_sup + 3 eps mean
  shares n_sup / (H W), n_clip / (H W): exact counts, one division, one narrowing 2 eps share
  dL/dD = (c psi) / A, c = lambda / n_sup narrowed once                           3 eps |dL/dD| + |c / A| dpsi
  dL/dA = -(dL/dD) (D / A)                                                        5 eps |dL/dA| + |c / A| |D / A| dpsi
Every quantity is held to max(2 e_ref, its bar), e_ref = |float32 restatement - float64|.

Fragile sets:
  F3    a supervised pixel whose e lies within de of 0: the sign (it matters in the linear zone only, i.e. when tau is
        within de of 0; kept as lidar_ref has it); removed from both gradients, capped at 1 % of the pixels.
  clip  a candidate with |a - clip| <= de + dclip would change n_sup and with it EVERY gradient: the inputs must have
        none.  inputs() builds them from copies of lidar_ref.inputs(case) and pushes every candidate whose a lies
        within 1e-3 m of its clip to 2e-3 m from it (de is about 1e-6 m at these depths): no cap is involved, the
        count is asserted to be zero.
Parameters of the bar cases: huber_abs 0.1, huber_rel 0.01, clip_abs 0.25, clip_rel 0.01 (lidar_ref's offsets run from
+-0.05 to +-0.4 m over 0.5 .. 10 m: every case with candidates beyond a handful has pixels in all three branches).

Exact cases (exact_case()): acc == 1, z_L a power of two, tau = z_L / 8 (huber_abs 0, huber_rel 1/8) and
clip = 1 + z_L / 4 dyadic, e a small multiple of 1/16 -- every per-pixel value and both f64 sums are exact in any
order, so the reference is the formulas in numpy float32 and is met bit for bit.  They hold pixels at exactly
a == clip (kept: the rule is >), at exactly a == tau (both branches give rho = tau / 2 and psi = +-1 there: which one
the kernel takes is unobservable), with e == 0, and beyond the clip.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

import lidar_ref as L

F64 = torch.float64
EPS = L.EPS
INF = float("inf")
f32 = np.float32
HUBER_ABS, HUBER_REL = float(f32(0.1)), float(f32(0.01))
CLIP_ABS, CLIP_REL = float(f32(0.25)), float(f32(0.01))
PARAMS = dict(huber_abs=HUBER_ABS, huber_rel=HUBER_REL, clip_abs=CLIP_ABS, clip_rel=CLIP_REL)
IDENTITY = dict(huber_abs=0.0, huber_rel=0.0, clip_abs=INF, clip_rel=0.0)
CLIP_MARGIN = 1e-3
TILE_W, TILE_H = 64, 16       # the kernel's tile: where filter_image() puts its seam and halo-only features


# ---- the occlusion filter ------------------------------------------------------------------------------------------
def filter32(img, radius, tol):
    """(filtered [H,W] float32, kept, removed): the contract of gsr_lidar_occlusion_filter."""
    z = np.ascontiguousarray(img, dtype=f32)
    H, W = z.shape
    with np.errstate(invalid="ignore"):
        valid = z > 0
    cand = np.where(valid, z, f32(np.inf))                 # what takes part in the minimum
    out = np.zeros((H, W), f32)
    t = f32(tol)
    kept = removed = 0
    with np.errstate(invalid="ignore"):
        for y, x in zip(*np.nonzero(valid)):
            zmin = cand[max(y - radius, 0):min(y + radius, H - 1) + 1, max(x - radius, 0):min(x + radius, W - 1) + 1].min()
            v = z[y, x]
            if zmin < f32(np.inf) and f32(v - zmin) > f32(t * v):
                removed += 1
            else:
                out[y, x] = v
                kept += 1
    return out, kept, removed


def filter_ops(img, radius, tol):
    """The filter in Torch ops of the image's dtype and device; returns the filtered image only."""
    z = img.reshape(img.shape[-2], img.shape[-1])
    inf = torch.full_like(z, INF)
    valid = z > 0
    cand = torch.where(valid, z, inf)
    zmin = -Fn.max_pool2d(-cand[None, None], 2 * radius + 1, stride=1, padding=radius)[0, 0]
    removed = valid & (zmin < inf) & ((z - zmin) > torch.as_tensor(tol, dtype=z.dtype, device=z.device) * z)
    return torch.where(valid & ~removed, z, torch.zeros_like(z)).reshape(img.shape)


@functools.lru_cache(maxsize=None)
def filter_image(H, W, seed=0):
    """A structured LiDAR image, float32: a far plane (7 .. 9 m) with dense returns; over x + 0.3 y < 0.45 W a near
    surface (2 .. 2.5 m) with returns on every third pixel in x and y, the far plane showing through between them --
    its slanted edge crosses the tile seams; a sprinkling of 0, negative, NaN and +inf entries; and, where the image is
    large enough, lone near returns (1 m) in the far region one pixel OUTSIDE each of the four borders of the tile at
    (TILE_W, TILE_H): they reach that tile through its halo only."""
    rng = np.random.default_rng(1000 + 7 * H + W + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = rng.uniform(7.0, 9.0, (H, W))
    near = (xx + 0.3 * yy < 0.45 * W) & (xx % 3 == 0) & (yy % 3 == 0)
    z = np.where(near, rng.uniform(2.0, 2.5, (H, W)), z).astype(f32)
    if H * W >= 15:
        flat = z.reshape(-1)
        idx = rng.permutation(H * W)[:max(4, H * W // 40)]
        for j, i in enumerate(idx):
            flat[i] = (0.0, -1.5, np.nan, np.inf)[j % 4]
    if W >= 2 * TILE_W + 2 and H >= 2 * TILE_H + 2:
        x0, y0 = TILE_W, TILE_H
        for (y, x) in ((y0 + 4, x0 - 1), (y0 + 9, x0 + TILE_W), (y0 - 1, x0 + 30), (y0 + TILE_H, x0 + 45)):
            z[y, x] = 1.0
    return z


# ---- the robust loss -------------------------------------------------------------------------------------------------
def robust_forward_ops(D, A, zl, acc_min, lam, huber_abs, huber_rel, clip_abs, clip_rel):
    """(loss, mean a, supervised share, clipped share) on tensors of one dtype and shape; differentiable in D and A."""
    cand = (zl > 0) & (A >= acc_min)
    safe = torch.where(cand, A, torch.ones_like(A))
    e = torch.where(cand, D / safe - zl, torch.zeros_like(D))
    a = e.abs()
    tau = huber_abs + huber_rel * zl
    clip = clip_abs + clip_rel * zl
    clipped = cand & (a > clip)
    sup = cand & ~clipped
    quad = sup & (a < tau)
    safe_tau = torch.where(quad, tau, torch.ones_like(tau))
    rho = torch.where(quad, 0.5 * a * (a / safe_tau), a - 0.5 * tau)
    rho = torch.where(sup, rho, torch.zeros_like(rho))
    n = sup.sum()
    nf = n.clamp_min(1).to(D.dtype)
    mean_rho = rho.sum() / nf
    mean = torch.where(sup, a, torch.zeros_like(a)).sum() / nf
    return lam * mean_rho, mean.detach(), n.to(D.dtype) / D.numel(), clipped.sum().to(D.dtype) / D.numel()


def robust_ops(depth, acc, lidar, acc_min=L.ACC_MIN, lam=L.LAMBDA, huber_abs=0.0, huber_rel=0.0, clip_abs=INF,
               clip_rel=0.0, dtype=F64):
    """{loss, mean, share, clip_share, grad_depth, grad_acc} of the robust depth loss, gradients from autograd."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    D, A, zl = t(depth).clone().requires_grad_(True), t(acc).clone().requires_grad_(True), t(lidar)
    loss, mean, share, cshare = robust_forward_ops(D, A, zl, acc_min, lam, huber_abs, huber_rel, clip_abs, clip_rel)
    gD, gA = torch.autograd.grad(loss, [D, A], allow_unused=True)
    z = lambda g: (torch.zeros_like(D) if g is None else g).detach()  # noqa: E731
    return dict(loss=loss.detach(), mean=mean.detach(), share=share.detach(), clip_share=cshare.detach(),
                grad_depth=z(gD), grad_acc=z(gA))


def pixel_terms(depth, acc, lidar, acc_min, huber_abs, huber_rel, clip_abs, clip_rel):
    """The per-pixel quantities in float64: masks (cand, sup, clipped, quad, lin), q, e, a, tau, clip, psi, rho."""
    D, A, zl = (torch.as_tensor(np.asarray(v), dtype=F64) for v in (depth, acc, lidar))
    cand = (zl > 0) & (A >= acc_min)
    q = torch.where(cand, D / torch.where(cand, A, torch.ones_like(A)), torch.zeros_like(D))
    e = torch.where(cand, q - zl, torch.zeros_like(D))
    a = e.abs()
    tau, clip = huber_abs + huber_rel * zl, clip_abs + clip_rel * zl
    clipped = cand & (a > clip)
    sup = cand & ~clipped
    quad = sup & (a < tau)
    lin = sup & ~quad
    psi = torch.where(quad, e / torch.where(quad, tau, torch.ones_like(tau)), torch.sign(e))
    psi = torch.where(sup, psi, torch.zeros_like(psi))
    rho = torch.where(quad, 0.5 * a * a / torch.where(quad, tau, torch.ones_like(tau)), a - 0.5 * tau)
    rho = torch.where(sup, rho, torch.zeros_like(rho))
    return dict(D=D, A=A, zl=zl, cand=cand, sup=sup, clipped=clipped, quad=quad, lin=lin, q=q, e=e, a=a, tau=tau,
                clip=clip, psi=psi, rho=rho)


def bars(truth, x, p):
    """Bars and fragile sets (module docstring).  truth: the float64 robust_ops dict; x: the inputs; p: the four
    parameters."""
    t = pixel_terms(x["depth"], x["acc"], x["lidar"], x["acc_min"], **p)
    zero = torch.zeros_like(t["D"])
    cand, sup, quad, lin = t["cand"], t["sup"], t["quad"], t["lin"]
    de = torch.where(cand, EPS * (t["q"].abs() + t["e"].abs()), zero)
    dtau, dclip = 2 * EPS * t["tau"], 2 * EPS * t["clip"]
    psi, rho, tau = t["psi"].abs(), t["rho"], t["tau"]
    safe_tau = torch.where(tau > 0, tau, torch.ones_like(tau))
    dpsi_q = de / safe_tau + dtau / safe_tau + EPS * psi
    near_tau = lin & (tau > 0) & ((t["a"] - tau) <= de + dtau)
    dpsi = torch.where(quad | near_tau, dpsi_q, zero)
    drho = torch.where(quad, psi * de + 0.5 * psi * psi * dtau + 2 * EPS * rho,
                       torch.where(lin, de + 0.5 * dtau + EPS * rho, zero))
    n = max(int(sup.sum()), 1)
    lam = abs(float(x["lam"]))
    dmean_rho = float(drho.sum()) / n + 3 * EPS * float(rho.sum()) / n
    dmean = float(torch.where(sup, de, zero).sum()) / n + 3 * EPS * float(truth["mean"])
    c_over_A = torch.where(sup, (lam / n) / torch.where(sup, t["A"], torch.ones_like(zero)), zero)
    bar = dict(loss=lam * dmean_rho + EPS * abs(float(truth["loss"])), mean=dmean,
               share=2 * EPS * float(truth["share"]), clip_share=2 * EPS * float(truth["clip_share"]),
               grad_depth=3 * EPS * truth["grad_depth"].abs() + c_over_A * dpsi,
               grad_acc=5 * EPS * truth["grad_acc"].abs() + c_over_A * t["q"].abs() * dpsi)
    return dict(bar=bar, F3=sup & (t["e"].abs() <= de), clip_fragile=cand & ((t["a"] - t["clip"]).abs() <= de + dclip),
                terms=t, de=de)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """lidar_ref.inputs(case), copied, with every candidate pixel whose a lies within CLIP_MARGIN of its clip pushed to
    2 CLIP_MARGIN from it (on the side it was on); the lidar_ref arrays themselves are left alone."""
    src = L.inputs(case)
    x = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in src.items()}
    t = pixel_terms(x["depth"], x["acc"], x["lidar"], x["acc_min"], **PARAMS)
    close = (t["cand"] & ((t["a"] - t["clip"]).abs() < CLIP_MARGIN)).numpy()
    if close.any():
        a, clip, e = t["a"].numpy(), t["clip"].numpy(), t["e"].numpy()
        target = clip + np.where(a > clip, 2 * CLIP_MARGIN, -2 * CLIP_MARGIN)
        D = x["acc"].astype(np.float64) * (x["lidar"].astype(np.float64) + np.where(e < 0, -1.0, 1.0) * target)
        x["depth"] = np.where(close, D, x["depth"].astype(np.float64)).astype(f32)
    return x


@functools.lru_cache(maxsize=None)
def reference(case):
    """Float64 truth, float32 yardstick, final bars, the pixels compared and the fragile counts of one of
    lidar_ref.CASES at PARAMS."""
    x = inputs(case)
    args = (x["depth"], x["acc"], x["lidar"], x["acc_min"], x["lam"])
    t = robust_ops(*args, **PARAMS)
    y32 = robust_ops(*args, **PARAMS, dtype=torch.float32)
    b = bars(t, x, PARAMS)
    bar, er = {}, {}
    for k in KEYS:
        er[k] = (y32[k].to(F64) - t[k]).abs()
        bar[k] = torch.maximum(2 * er[k], torch.as_tensor(b["bar"][k], dtype=F64))
    tm = b["terms"]
    return dict(truth=t, f32=y32, bar=bar, eref=er, keep=~b["F3"], fragile_pixels=int(b["F3"].sum()),
                clip_fragile=int(b["clip_fragile"].sum()), n_cand=int(tm["cand"].sum()), n_sup=int(tm["sup"].sum()),
                n_quad=int(tm["quad"].sum()), n_lin=int(tm["lin"].sum()), n_clip=int(tm["clipped"].sum()), terms=tm)


KEYS = ("loss", "mean", "share", "clip_share", "grad_depth", "grad_acc")


def loss_ratios(got, ref):
    """worst |got - truth| / bar per quantity; got: {loss, mean, share, clip_share: float, grad_depth, grad_acc: float64
    tensor}."""
    out = {}
    for k in ("grad_depth", "grad_acc"):
        d = (got[k].to(F64).reshape(ref["truth"][k].shape) - ref["truth"][k]).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, 1e30))
        out[k] = L._ratio(d.numpy(), ref["bar"][k].numpy(), ref["keep"].numpy())
    for k in ("loss", "mean", "share", "clip_share"):
        out[k] = L._ratio(abs(float(got[k]) - float(ref["truth"][k])), float(ref["bar"][k]), True)
    return out


# ---- exact cases -----------------------------------------------------------------------------------------------------
EXACT = dict(huber_abs=0.0, huber_rel=0.125, clip_abs=1.0, clip_rel=0.25)
EXACT_SHAPES = ((3, 5), (37, 61))
EXACT_LAMBDA = 0.5


@functools.lru_cache(maxsize=None)
def exact_case(H, W):
    """Inputs (acc == 1, z_L in {1, 2, 4, 8} with holes, e from a table that holds 0, +-tau, +-clip, values inside each
    zone and beyond the clip) and the reference {out4, grad_depth, grad_acc} in numpy float32."""
    rng = np.random.default_rng(31 * H + W)
    zl = (2.0 ** rng.integers(0, 4, (H, W))).astype(f32)
    zl.reshape(-1)[::11] = 0.0
    tau, clip = zl / 8, 1 + zl / 4
    kind = rng.integers(0, 9, (H, W))
    kind.reshape(-1)[:9] = np.arange(9)[:min(9, H * W)]            # every kind at least once
    sgn = (rng.integers(0, 2, (H, W)) * 2 - 1).astype(np.float64)
    table = [0 * tau, tau, clip, tau / 2, tau / 4, tau + 1 / 16, clip - 1 / 16, clip + 1 / 16, clip + 3.0]
    a = np.choose(kind, table)
    e = (sgn * a).astype(f32)
    A = np.ones((H, W), f32)
    D = (zl + e).astype(f32)
    assert np.array_equal(D.astype(np.float64), zl.astype(np.float64) + sgn * a)
    # the formulas in float32, every operation exact or a single IEEE operation on exact operands
    cand = zl > 0
    q = D / A
    ee = (q - zl).astype(f32)
    aa = np.abs(ee)
    tau32 = (f32(EXACT["huber_abs"]) + f32(EXACT["huber_rel"]) * zl).astype(f32)
    clip32 = (f32(EXACT["clip_abs"]) + f32(EXACT["clip_rel"]) * zl).astype(f32)
    clipped = cand & (aa > clip32)
    sup = cand & ~clipped
    quad = sup & (aa < tau32)
    with np.errstate(all="ignore"):
        rho = np.where(quad, f32(0.5) * aa * (aa / np.where(quad, tau32, f32(1))), aa - f32(0.5) * tau32).astype(f32)
        psi = np.where(quad, ee / np.where(quad, tau32, f32(1)), np.sign(ee)).astype(f32)
    n = int(sup.sum())
    rs, as_ = float(rho[sup].astype(np.float64).sum()), float(aa[sup].astype(np.float64).sum())   # exact sums
    lam = f32(EXACT_LAMBDA)
    out4 = np.array([lam * f32(rs / n), f32(as_ / n), f32(n / (H * W)), f32(int(clipped.sum()) / (H * W))], f32)
    c = f32(float(lam) / n)
    gd = np.where(sup & (psi != 0), (c * psi) / A, f32(0)).astype(f32)
    ga = (-gd * q).astype(f32)
    ga = np.where(gd != 0, ga, f32(0)).astype(f32)
    seen = dict(zero_e=int((sup & (ee == 0)).sum()), at_tau=int((sup & (aa == tau32)).sum()),
                at_clip=int((sup & (aa == clip32)).sum()), clipped=int(clipped.sum()), quad=int(quad.sum()))
    return dict(H=H, W=W, depth=D, acc=A, lidar=zl, acc_min=0.5, lam=EXACT_LAMBDA, out4=out4, grad_depth=gd,
                grad_acc=ga, seen=seen, sup=sup)
