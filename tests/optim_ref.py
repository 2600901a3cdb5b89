"""Plain-Torch restatement of the optimiser tail (csrc/optimizer.hip) with the dtype as a parameter, on the CPU.

  * the getters of GaussianModel (include/gs/gs/gaussian.cuh:40-54): exp, sigmoid, torch.nn.functional.normalize, cat,
    and their backward THROUGH AUTOGRAD (no hand-written chain rule: nothing here shares a formula with the kernels);
  * one step of torch::optim::Adam as the reference configures it (src/gs/gaussian.cu:396-428), the formula quoted above
    `adam1` in optimizer.hip, with betas / eps / learning rates as Python doubles and the bias corrections in double;
  * `model_step_ref`: chain rule -> Adam on the six groups -> activations of the updated parameters.

Run in float64 it is the truth the kernels are held to; run in float32 it is the yardstick e_ref (the reference's own
arithmetic at the kernels' precision).  `bars` turns the two into the per-element bar

    max(2 * e_ref, floor),   floor = K * 2^-23 * magnitude + (what the floors of the quantities it is made from become)

The factor 2 is the house rule of test_gpu_simi.py: the kernel's order of operations is not Torch's, so it may err by as
much as Torch in the other direction.  K counts float32 roundings along the longest chain between the inputs and the
quantity, one 2^-23 each (twice the unit roundoff); a constant rounded from double is one rounding, expf two (a
library function good to one ulp).  The magnitude is what those roundings scale with, in float64.  Per quantity:

  scales = exp(x)             K = 2  (expf)                                          magnitude exp(x)
  opacity s = 1/(1+exp(-x))   K = 4  (expf, add, divide)                             magnitude s
  rotation y = q/max(|q|,c)   K = 7  (square, three adds, root, reciprocal, multiply) magnitude |y_k|
  shs = cat(f_dc, f_rest)     exact
  dL/dscaling = g exp(x)      K = 3  (expf, multiply)                                magnitude |g| exp(x)
  dL/dopacity = g s (1 - s)   K = 7  (s: 4; 1 - s, two multiplies: 3)                magnitude |g| s: the absolute rounding
                              of s, 4 * 2^-23 * s, passes unchanged into 1 - s, so the error scales with |g| s ((1-s) + s),
                              not with the value |g| s (1-s) -- a saturated opacity is ill-conditioned and the bar says so
  dL/drotation_k              K = 12 (y_k: 5 half-units; y.g: 9 over sum_j |y_j g_j|; times y_k, subtract, times 1/|q| with
                              its own 4 + 1: 21 half-units <= 12 units)              magnitude (|g_k| + |y_k| sum_j |y_j g_j|)
                              / max(|q|, 1e-12); sum_j |y_j g_j| and not |y.g|: the roundings of the dot product do not
                              cancel where its terms do.  The clamped branch (g * 1e12: K = 2) is inside the same bar.
  dL/dxyz, dL/df_dc, dL/df_rest   exact (copies)
  exp_avg                     K = 3  (constant, multiply, add)      magnitude |m| b1 + |g| (1-b1), plus (1-b1) * floor(g)
  exp_avg_sq                  K = 4  (g g, constant, multiply, add) magnitude v b2 + g g (1-b2), plus 2 |g| (1-b2) floor(g)
  update p_new - p_old        K = 3 + 4: step_size (constant), divide, multiply on |u| = step_size |m'| / denom, and root,
                              1/sqrt(bc2) (constant), multiply, add on denom; plus step_size floor(m') / denom, plus
                              |u| / denom * floor(v') / (2 sqrt(v') sqrt(bc2)), plus half an ulp (2^-24) of
                              max(|p_old|, |p_new|) for the final subtraction
  next activations            their own K as above on the updated parameter, plus the derivative of the activation times
                              floor(update) (for the quaternion (d_k + |y_k| sum_j |y_j| d_j) / |q|)

No element is masked.  The generators keep float32 in its normal range; an element for which some float64 intermediate
is non-zero and below 64 * FLT_MIN (or above FLT_MAX / 64) cannot be judged -- float32 goes subnormal or overflows where
float64 does not -- and `judgeable` drops it from both sides.  At most 0.1 % of a case may be dropped (DROP_CAP).
"""
import math

import numpy as np
import torch

GROUPS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")
ACTS = ("scales", "rotations", "opacities", "shs")
EPS32 = 2.0 ** -23
FLT_MIN = 2.0 ** -126
FLT_MAX = 3.4028234663852886e38
DROP_CAP = 1e-3
NORM_EPS = 1e-12
K = dict(scales=2, opacities=4, rotations=7, g_scaling=3, g_opacity=7, g_rotation=12, exp_avg=3, exp_avg_sq=4,
         update_own=3, denom=4)
BETAS = (0.9, 0.999)
STEPS = (1, 2, 10, 1000, 30000)
EPSES = (1e-15, 1e-8)
# the grid of test_gpu_optim_ref64.py (kept here so that the CPU anchor can hold every generator to the drop cap)
GRID_MS = (1, 2, 4, 9, 16)
GRID_PS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)
GRID = [(M, P) for M in GRID_MS for P in GRID_PS]
P_LARGE = 200003


def grid_hyper(i):
    """(step, eps) of grid case i: every step count meets both eps."""
    return STEPS[i % 5], EPSES[(i // 5) % 2]


def default_lrs():
    """The learning rates of GaussianParameters.param_groups() (config/basic_common.yaml:54-62), as the float32 values the
    C ABI receives, widened back to double."""
    return [float(np.float32(x)) for x in (0.0005, 0.001, 0.001 / 20.0, 0.0025, 0.0025, 0.025)]


# ---- the operations ------------------------------------------------------------------------------------------------
def activations(scaling, rotation, opacity, f_dc, f_rest):
    """(scales, rotations, opacities, shs) as GaussianModel's getters compute them."""
    return (torch.exp(scaling), torch.nn.functional.normalize(rotation), torch.sigmoid(opacity),
            torch.cat([f_dc, f_rest], 1))


def activations_backward(raw, ups, dtype):
    """Autograd through `activations`: raw {scaling, rotation, opacity, f_dc, f_rest}, ups (g_scales, g_rot, g_opac,
    g_shs) -> (activated values, {group: gradient w.r.t. the raw leaf})."""
    names = ("scaling", "rotation", "opacity", "f_dc", "f_rest")
    leaves = [raw[k].detach().to(dtype).clone().requires_grad_(True) for k in names]
    acts = activations(*leaves)
    grads = torch.autograd.grad(list(acts), leaves, [u.to(dtype) for u in ups], allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    return tuple(a.detach() for a in acts), dict(zip(names, grads))


def adam_step(p, g, m, v, lr, step, betas=BETAS, eps=1e-15):
    """torch::optim::Adam::step (no weight decay, no amsgrad) on tensors of one dtype; every hyperparameter is a Python
    double, as the options of torch::optim are.  Returns (p_new, exp_avg, exp_avg_sq)."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m = m * b1 + g * (1.0 - b1)
    v = v * b2 + g * g * (1.0 - b2)
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def model_step_ref(case, dtype, lrs=None, step=1, betas=BETAS, eps=1e-15):
    """The optimiser tail on `case` (see make_case: float32 CPU tensors) in `dtype`.  Returns a dict of dicts:
    act (activations of the old parameters), g (raw-space gradients), m, v, p (new parameters), update (p_new - p_old,
    formed in float64 from the two values AT `dtype`), next (activations of the new parameters); all float64."""
    lrs = default_lrs() if lrs is None else lrs
    raw = {k: case["p"][k].to(dtype) for k in GROUPS}
    act, g = activations_backward(raw, [case["ups"][k] for k in ("scales", "rotations", "opacities", "shs")], dtype)
    g["xyz"] = case["ups"]["xyz"].to(dtype)
    out = dict(act=dict(zip(ACTS, act)), g=g, m={}, v={}, p={}, update={})
    for k, lr in zip(GROUPS, lrs):
        out["p"][k], out["m"][k], out["v"][k] = adam_step(raw[k], g[k], case["m"][k].to(dtype), case["v"][k].to(dtype),
                                                         lr, step, betas, eps)
        out["update"][k] = out["p"][k].double() - raw[k].double()
    n = out["p"]
    out["next"] = dict(zip(ACTS, activations(n["scaling"], n["rotation"], n["opacity"], n["f_dc"], n["f_rest"])))
    return {a: {k: t.double() for k, t in d.items()} for a, d in out.items()}


# ---- inputs --------------------------------------------------------------------------------------------------------
def _decades(gen, shape, lo, hi):
    """+-10^U(lo, hi)."""
    mag = 10.0 ** (lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64))
    return mag * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)


def make_case(P, M, seed, step=1, quats="mixed"):
    """Float32 CPU inputs of one optimiser step for P Gaussians with M SH coefficients per channel.

    Upstream gradients are 0 or +-[1e-12, 1e8] (log-uniform): 10 % of the elements are exact zeros, ~15 % of the
    Gaussians are culled (every gradient of the row zero; row 0 always when P >= 2), and every other culled row has zero
    moments as well (+0: a kernel may turn -0 into +0).  Raw scaling in [-12, 6], its gradient from 1e-15 exp(-x)
    where that is above 1e-12 (so that the square of g exp(x) times 1 - beta2 stays a normal float32); raw opacity in [-6, 6] with 10 % saturated (8 <= |x| <= 16, whose
    gradients start at 1e-6 so that g s (1-s) stays a normal float32).  Quaternions ("mixed"): unit, scaled by 1e-6 ...
    1e4, |q| = {0.3, 0.9, 1.1, 3} * 1e-12 and exactly zero; the rotation gradients lie in [1e-14 |q|, 1e14 |q|] (at most
    1e2 on the clamped branch) so that the squares of g / |q| stay normal and finite in float32.  Moments (zero at step 1) are the float64 raw-space
    gradient times a factor in +-[0.1, 1.5] (squared: [0.3, 2]) times the bias factor 1 - beta^(step-1): the decade
    of the gradient."""
    gen = torch.Generator().manual_seed(1000003 * seed + 1009 * P + M)
    r64 = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    p = dict(xyz=torch.randn(P, 3, generator=gen, dtype=torch.float64) * 10,
             f_dc=torch.randn(P, 1, 3, generator=gen, dtype=torch.float64),
             f_rest=torch.randn(P, M - 1, 3, generator=gen, dtype=torch.float64) * 0.1,
             scaling=-12 + 18 * r64(P, 3), opacity=-6 + 12 * r64(P, 1))
    sat = r64(P, 1) < 0.1
    p["opacity"] = torch.where(sat, (8 + 8 * r64(P, 1)) * (torch.randint(0, 2, (P, 1), generator=gen) * 2 - 1), p["opacity"])
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=gen, dtype=torch.float64))
    kind = torch.randint(0, 8, (P,), generator=gen) if quats == "mixed" else torch.zeros(P, dtype=torch.long)
    scale = torch.ones(P, dtype=torch.float64)
    scale = torch.where(kind == 1, 10.0 ** (-6 + 10 * r64(P)), scale)
    scale = torch.where(kind == 2, 0.5 + 1.5 * r64(P), scale)
    for k, f in ((3, 0.3e-12), (4, 0.9e-12), (5, 1.1e-12), (6, 3e-12), (7, 0.0)):
        scale = torch.where(kind == k, torch.full_like(scale, f), scale)
    p["rotation"] = q * scale[:, None]
    p = {k: t.float() for k, t in p.items()}
    qn = p["rotation"].double().norm(dim=1, keepdim=True)
    ups = dict(xyz=_decades(gen, (P, 3), -12, 8), scales=_decades(gen, (P, 3), -12, 8),
               opacities=torch.where(sat, _decades(gen, (P, 1), -6, 8), _decades(gen, (P, 1), -12, 8)),
               shs=_decades(gen, (P, M, 3), -12, 8))
    lo = (-15 - p["scaling"].double() / math.log(10.0)).clamp(min=-12)
    ups["scales"] = 10.0 ** (lo + (8 - lo) * r64(P, 3)) * (torch.randint(0, 2, (P, 3), generator=gen) * 2 - 1)
    hi = torch.log10((1e14 * qn.clamp(min=NORM_EPS)).clamp(max=1e8)).expand(P, 4)
    lo = (-14 + torch.log10(qn.clamp(min=NORM_EPS))).clamp(min=-12).expand(P, 4)
    ups["rotations"] = 10.0 ** (lo + (hi - lo) * r64(P, 4)) * (torch.randint(0, 2, (P, 4), generator=gen) * 2 - 1)
    culled = r64(P) < 0.15
    if P >= 2:
        culled[0] = True
    for k, t in ups.items():
        t = torch.where(r64(t.shape) < 0.1, torch.zeros_like(t), t)
        ups[k] = torch.where(culled.view(-1, *([1] * (t.dim() - 1))), torch.zeros_like(t), t).float()
    case = dict(P=P, M=M, p=p, ups=ups, culled=culled, m={k: torch.zeros_like(p[k]) for k in GROUPS},
                v={k: torch.zeros_like(p[k]) for k in GROUPS})
    if step > 1:
        g = model_step_ref(case, torch.float64)["g"]
        f1, f2 = 1.0 - BETAS[0] ** (step - 1), 1.0 - BETAS[1] ** (step - 1)
        still = culled & (torch.arange(P) % 2 == 0)   # culled AND never moved: zero moments
        for k in GROUPS:
            gg = torch.where(g[k] == 0, _decades(gen, g[k].shape, -8, -4), g[k])
            a = (0.1 + 1.4 * r64(gg.shape)) * (torch.randint(0, 2, gg.shape, generator=gen) * 2 - 1)
            gone = still.view(-1, *([1] * (gg.dim() - 1)))
            case["m"][k] = torch.where(gone, torch.zeros_like(gg), gg * a * f1).float()
            case["v"][k] = torch.where(gone, torch.zeros_like(gg), gg * gg * (0.3 + 1.7 * r64(gg.shape)) * f2).float()
    return case


# ---- the bar -------------------------------------------------------------------------------------------------------
def _adam_terms(case, r64, lrs, step, betas, eps):
    """float64 pieces of the Adam step per group, from the float32 inputs and the float64 raw-space gradient."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    out = {}
    for k, lr in zip(GROUPS, lrs):
        g, m, v = r64["g"][k], case["m"][k].double(), case["v"][k].double()
        denom = r64["v"][k].sqrt() / math.sqrt(bc2) + eps
        out[k] = dict(g=g, t_m=(m * b1, g * (1 - b1)), t_v=(v * b2, g * g, g * g * (1 - b2)), ss=lr / bc1,
                      c=1.0 / math.sqrt(bc2), denom=denom, ratio=r64["m"][k] / denom)
    return out


def judgeable(case, r64, lrs=None, step=1, betas=BETAS, eps=1e-15):
    """{group: bool tensor}: False where a float64 intermediate is non-zero below 64 * FLT_MIN or above FLT_MAX / 64
    (float32 would leave its normal range there).  A quaternion is judged or dropped as a whole."""
    lrs = default_lrs() if lrs is None else lrs
    bad = lambda t: ((t != 0) & (t.abs() < 64 * FLT_MIN)) | (t.abs() > FLT_MAX / 64)  # noqa: E731
    terms = _adam_terms(case, r64, lrs, step, betas, eps)
    ok = {}
    for k in GROUPS:
        t = terms[k]
        b = bad(t["g"]) | bad(r64["m"][k]) | bad(r64["v"][k]) | bad(t["ratio"]) | bad(t["ratio"] * t["ss"])
        for x in t["t_m"] + t["t_v"]:
            b |= bad(x)
        ok[k] = ~b
    q = case["p"]["rotation"].double()
    whole = ~(bad(q * q).any(1, keepdim=True) | ~ok["rotation"].all(1, keepdim=True))
    ok["rotation"] = whole.expand_as(q).clone()
    return ok


def dropped_fraction(ok):
    n = sum(int(t.numel()) for t in ok.values())
    return (sum(int((~t).sum()) for t in ok.values()) / n) if n else 0.0


def floors(case, r64, lrs=None, step=1, betas=BETAS, eps=1e-15):
    """The K * 2^-23 * magnitude part of every bar (module docstring), float64, same layout as model_step_ref."""
    lrs = default_lrs() if lrs is None else lrs
    b1, b2 = betas
    E = EPS32
    p = {k: case["p"][k].double() for k in GROUPS}
    ups = {k: t.double() for k, t in case["ups"].items()}
    act, nxt = r64["act"], r64["next"]
    f = dict(act={}, g={}, m={}, v={}, update={}, next={})
    f["act"] = dict(scales=K["scales"] * E * act["scales"], opacities=K["opacities"] * E * act["opacities"],
                    rotations=K["rotations"] * E * act["rotations"].abs(), shs=torch.zeros_like(act["shs"]))
    y = act["rotations"]
    qn = p["rotation"].norm(dim=1, keepdim=True).clamp(min=NORM_EPS)
    dot_abs = (y * ups["rotations"]).abs().sum(1, keepdim=True)
    f["g"] = dict(xyz=torch.zeros_like(p["xyz"]), f_dc=torch.zeros_like(p["f_dc"]), f_rest=torch.zeros_like(p["f_rest"]),
                  scaling=K["g_scaling"] * E * (ups["scales"] * act["scales"]).abs(),
                  opacity=K["g_opacity"] * E * ups["opacities"].abs() * act["opacities"],
                  rotation=K["g_rotation"] * E * (ups["rotations"].abs() + y.abs() * dot_abs) / qn)
    terms = _adam_terms(case, r64, lrs, step, betas, eps)
    for k in GROUPS:
        t, dg = terms[k], f["g"][k]
        f["m"][k] = K["exp_avg"] * E * (t["t_m"][0].abs() + t["t_m"][1].abs()) + (1 - b1) * dg
        f["v"][k] = K["exp_avg_sq"] * E * (t["t_v"][0] + t["t_v"][2]) + 2 * t["g"].abs() * (1 - b2) * dg
        root = r64["v"][k].sqrt()
        droot = torch.where(root > 0, f["v"][k] / (2 * root.clamp(min=1e-300)), torch.zeros_like(root))
        ddenom = K["denom"] * E * t["denom"] + t["c"] * droot
        u = t["ss"] * t["ratio"].abs()
        f["update"][k] = (K["update_own"] * E * u + t["ss"] * f["m"][k] / t["denom"] + u * ddenom / t["denom"]
                          + 0.5 * E * torch.maximum(p[k].abs(), r64["p"][k].abs()))
    d = f["update"]
    yn = nxt["rotations"]
    qn2 = r64["p"]["rotation"].norm(dim=1, keepdim=True).clamp(min=NORM_EPS)
    f["next"] = dict(
        scales=nxt["scales"] * (K["scales"] * E + d["scaling"]),
        opacities=nxt["opacities"] * (K["opacities"] * E + (1 - nxt["opacities"]) * d["opacity"]),
        rotations=K["rotations"] * E * yn.abs() + (d["rotation"] + yn.abs() * (yn.abs() * d["rotation"]).sum(1, keepdim=True)) / qn2,
        shs=torch.cat([d["f_dc"], d["f_rest"]], 1))
    return f


def bars(case, r64, r32, **hyper):
    """{quantity: {name: (e_ref, bar)}}: e_ref = |float32 restatement - float64|, bar = max(2 e_ref, floor)."""
    fl = floors(case, r64, **hyper)
    out = {}
    for a in fl:
        out[a] = {}
        for k in fl[a]:
            e = (r32[a][k] - r64[a][k]).abs()
            out[a][k] = (e, torch.maximum(2 * e, fl[a][k]))
    return out


def worst_ratios(got, r64, bar, ok):
    """{quantity.name: (max err, max e_ref, max bar, max err / bar)} over the judged elements of what `got` holds."""
    act_ok = dict(scales=ok["scaling"], rotations=ok["rotation"], opacities=ok["opacity"],
                  shs=torch.cat([ok["f_dc"], ok["f_rest"]], 1))
    res = {}
    for a in got:
        for k, t in got[a].items():
            if a == "act":   # the activations of the OLD parameters do not pass through Adam: always judged
                keep = torch.ones_like(r64[a][k], dtype=torch.bool)
            else:
                keep = act_ok[k] if a == "next" else ok[k]
            if not bool(keep.any()):
                continue
            err = (t.double().cpu() - r64[a][k]).abs()[keep]
            e_ref, b = bar[a][k][0][keep], bar[a][k][1][keep]
            ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
            res["%s.%s" % (a, k)] = (float(err.max()), float(e_ref.max()), float(b.max()), float(ratio.max()))
    return res
