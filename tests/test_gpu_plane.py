"""GPU tests of the fused point-to-plane LiDAR loss on oriented surfels (csrc/surfel.hip, gsr_surfel_plane_loss;
loss.py, model.py, torch_next.cpp) against the float64 restatement of its definition (tests/plane_ref.py).

How close is close enough (no constant is picked).  As tests/test_gpu_simi.py: the yardstick is the restatement run in
float32 Torch ops on the same inputs; its distance e_ref to the float64 result is measured per quantity -- the four
outputs, every selected row of each of the three gradients -- and the HIP result may be

    max(2 * e_ref, K * eps32 * magnitude)

away from float64 (2: our order of operations is not Torch's, we may err as much in the other direction; the second
term is the floor where Torch happens to be exact).  eps32 = 2^-23, twice the unit roundoff.  K counts the float32
roundings between the inputs and a result; the magnitude is what their relative errors scale with, in float64.

  e_i = n . v:  v = p - x (1), an entry of R(q) (at most two products, one sum, one difference: 4), the product (1),
      two additions (2): K_e = 8.  The entries of R are sums of monomials of q whose absolute values add up to at most
      N_j = 1 + 2 |q_j|^2, and the three products can cancel, so the absolute error of e_i scales with
      E_i = N_j (|v_x| + |v_y| + |v_z|), not with |e_i|.
  rho'_i:  exact (+-1) outside the knee; e_i / huber inside it, which magnifies the error of e_i by 1 / huber.  A
      point therefore weighs T_i = g_i (|rho'_i| + [inside the knee] E_i / huber) in the error of a sum of rho'.
  out4[1] = mean g rho:  the error of rho_i is at most that of e_i (|rho'| <= 1) plus rho's own two roundings (square
      and division, or one subtraction), the division by m (1) and a pairwise sum over m points:
      K = K_e + 3 + ceil(log2 m), magnitude mean_i g_i (E_i + rho_i).
  out4[2] = mean thinnest scale:  K = 1 + ceil(log2 n), magnitude the value.
  out4[3] = share of gated-in points:  an integer count (exact once the fragile points are gone) and one division:
      K = 1, magnitude the value.
  out4[0]:  two products and one addition on top of the larger of the two K above: K = max(K_1, K_2) + 3, magnitude
      lambda * magnitude_1 + lambda_flat * magnitude_2.
  grad_xyz[j] = -(lambda/m) A_j n_j:  K_e, the division by huber (1), a pairwise sum over the points that share the row
      (ceil(log2 of the largest share)), the entry of n (4), lambda/m, its product with A and with n (3):
      K_x = 16 + ceil(log2 max share); magnitude (lambda/m) N_j sum_{i->j} T_i.
  grad_rotation[j] = J^T (lambda/m) B_j:  one more product (rho' v) and a three-term entry of J^T b instead of n's:
      K_q = K_x + 2.  Every entry of J^T b is at most 4 max|q_j| (|b_x| + |b_y| + |b_z|):
      magnitude (lambda/m) 4 max|q_j| sum_{i->j} T_i (|v_x| + |v_y| + |v_z|)_i.
  grad_scaling[j][k*] = lambda_flat / n:  one division, K = 1, magnitude the value; the other two elements are 0.

Fragile points (plane_ref.analyse states the four rules) may land on the other side of a comparison in float32: they
are removed from the inputs of BOTH sides, and a case fails if that removes more than 1 % of its points (a cap, not a
tolerance; tests/test_plane_ref.py holds every case to it on the CPU).  Measured ratios of error to bar, and the check
that refuses each mutant, are recorded in DESIGN.md section 2.
"""
import functools
import json
import math

import pytest
import torch

import gs_livm_amd as G
import plane_ref as PR
import simi_ref
from arena import Arena, offsets
from gs_livm_amd import _capi

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
LAM = PR.LAM
DEV = "cuda:0"
SIZES = list(PR.CASES)
PIDS = ["abs", "huber-0.05-flat", "huber-0.08"]
QUANTITIES = ("loss", "mean_rho", "mean_thin", "gate_share", "gx", "gs", "gr")


@functools.lru_cache(maxsize=None)
def _inputs(m, n):
    return PR.case_inputs(m, n, DEV)


def _with_refs(c, params):
    """Adds the float64 truth, the float32 yardstick and the float64 facts the bars need to a dict of inputs."""
    args = (c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"])
    a = PR.analyse(*args, params)
    assert not bool(a["fragile"].any())
    n, mm = c["sel"].shape[0], c["points"].shape[0]
    huber = params[0]
    T = a["gate"].double() * (a["drho"].abs() + (a["knee"].double() * a["E"] / huber if huber > 0 else 0.0))
    zeros = torch.zeros(n, dtype=torch.float64, device=T.device)
    c.update(params=params, m=mm, n=n, facts=a, ref64=PR.reference(*args, params, torch.float64),
             ref32=PR.reference(*args, params, torch.float32),
             shares=torch.bincount(a["j"][a["gate"]], minlength=n),
             sumT=zeros.clone().index_add_(0, a["j"], T), sumTv=zeros.clone().index_add_(0, a["j"], T * a["v1"]))
    return c


@functools.lru_cache(maxsize=None)
def _case(m, n, pi):
    params = PR.PARAMS[pi]
    c = dict(_inputs(m, n))
    a = PR.analyse(c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"], params)
    removed = int(a["fragile"].sum())
    assert removed <= 0.01 * m, "%d of %d points are fragile" % (removed, m)
    c["points"] = c["points"][~a["fragile"]].contiguous()
    c["removed"] = removed
    return _with_refs(c, params)


def _bars(c):
    """Per quantity: (K, magnitude) as the module docstring derives them; scalars or one value per selected row."""
    a, (huber, _, lambda_flat), m, n = c["facts"], c["params"], c["m"], c["n"]
    g = a["gate"].double()
    lg = lambda v: math.ceil(math.log2(max(int(v), 1)))  # noqa: E731
    K1, K2 = 8 + 3 + lg(m), 1 + lg(n)
    M1 = float((g * (a["E"] + a["rho"])).sum() / m)
    M2 = float(c["ref64"]["out4"][2])
    Kx = 16 + lg(c["shares"].max())
    cm = LAM / m
    return {"loss": (max(K1, K2) + 3, LAM * M1 + lambda_flat * M2), "mean_rho": (K1, M1), "mean_thin": (K2, M2),
            "gate_share": (1, float(c["ref64"]["out4"][3])),
            "gx": (Kx, cm * a["N"] * c["sumT"]), "gr": (Kx + 2, cm * 4 * a["q"].abs().amax(1) * c["sumTv"]),
            "gs": (1, lambda_flat / n)}


def _compare(c, out4, gx, gs, gr):
    """error / bar per quantity (the worst selected row for a gradient), and e_ref, bar and error for the record."""
    a, b, sel, bars = c["ref64"], c["ref32"], c["sel"].long(), _bars(c)
    rec = {}
    for i, name in enumerate(QUANTITIES[:4]):
        K, mag = bars[name]
        e_ref = float((b["out4"][i] - a["out4"][i]).abs())
        bar = max(2 * e_ref, K * EPS32 * mag)
        err = float((out4[i].double() - a["out4"][i]).abs())
        rec[name] = dict(K=K, e_ref=e_ref, bar=bar, err=err, ratio=err / bar if bar > 0 else (0.0 if err == 0 else math.inf))
    for name, got in (("gx", gx), ("gs", gs), ("gr", gr)):
        K, mag = bars[name]
        e_ref = (b[name] - a[name]).index_select(0, sel).abs().amax(1)
        bar = torch.maximum(2 * e_ref, K * EPS32 * torch.as_tensor(mag, dtype=torch.float64, device=e_ref.device))
        err = (got.double() - a[name]).index_select(0, sel).abs().amax(1)
        ratio = torch.where(bar > 0, err / bar.clamp(min=1e-300),
                            torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        rec[name] = dict(K=K, e_ref=float(e_ref.max()), bar=float(bar.max()), err=float(err.max()), ratio=float(ratio.max()))
    return rec


def _check(c, out4, gx, gs, gr, what):
    """Holds one result (dense gradients) against float64 at the derived bars; prints every figure first."""
    rec = _compare(c, out4, gx, gs, gr)
    print(json.dumps(dict(what=what, m=c["m"], n=c["n"], P=c["P"], params=list(c["params"]), removed=c.get("removed"),
                          gated_in=int(c["facts"]["gate"].sum()), in_knee=int((c["facts"]["knee"] & c["facts"]["gate"]).sum()),
                          largest_share=int(c["shares"].max()), **{k: v for k, v in rec.items()})))
    for name in QUANTITIES:
        assert rec[name]["ratio"] <= 1.0, "%s: error at %.3g of its bar" % (name, rec[name]["ratio"])
    outside = torch.ones(c["P"], dtype=torch.bool, device=gx.device)
    outside[c["sel"].long()] = False
    for g in (gx, gs, gr):                       # rows outside the selection: exactly zero
        assert not bool(g[outside].any())
    return rec


def _run_capi(c, accumulate=False, fill=None, lam=LAM, params=None, points=None):
    P, dev = c["P"], c["xyz"].device
    huber, max_dist, lambda_flat = c["params"] if params is None else params
    if fill is None:
        gx, gs, gr = (torch.zeros((P, w), device=dev) for w in (3, 3, 4))
    else:
        gx, gs, gr = (f.clone() for f in fill)
    out4 = _capi.surfel_plane_loss(c["points"] if points is None else points, c["sel"], c["xyz"], c["scaling"],
                                   c["rotation"], lam, huber, max_dist, lambda_flat, gx, gs, gr, accumulate=accumulate)
    return out4, gx, gs, gr


@pytest.mark.parametrize("pi", range(3), ids=PIDS)
@pytest.mark.parametrize("m,n", SIZES)
def test_capi_matches_float64_at_the_derived_bar(m, n, pi, gpu_device):
    c = _case(m, n, pi)
    out4, gx, gs, gr = _run_capi(c)
    _check(c, out4, gx, gs, gr, "capi")
    # forward only: the same four numbers, no gradient buffer needed; any subset of the three gradients: the same rows
    huber, max_dist, lambda_flat = c["params"]
    args = (c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"], LAM, huber, max_dist, lambda_flat)
    assert torch.equal(_capi.surfel_plane_loss(*args), out4)
    only_r = torch.zeros_like(gr)
    assert torch.equal(_capi.surfel_plane_loss(*args, grad_rotation=only_r), out4) and torch.equal(only_r, gr)
    only_s = torch.zeros_like(gs)
    assert torch.equal(_capi.surfel_plane_loss(*args, grad_scaling=only_s), out4) and torch.equal(only_s, gs)


@pytest.mark.parametrize("m,n", [(65, 272), (2500, 16), (500, 8000)])
def test_both_sides_of_the_gate_and_of_the_knee_are_exercised(m, n, gpu_device):
    for pi in (1, 2):
        f = _case(m, n, pi)["facts"]
        share = float(f["gate"].double().mean())
        assert 0.1 < share < 0.9, share
        assert bool((f["knee"] & f["gate"]).any()) and bool((~f["knee"] & f["gate"]).any())
    assert int(_case(2500, 16, 0)["shares"].max()) >= 50           # records of one row in several staging tiles


@pytest.mark.parametrize("pi", range(3), ids=PIDS)
@pytest.mark.parametrize("m,n", [(7, 16), (65, 272), (2500, 16), (500, 8000)])
def test_accumulate_untouched_rows_and_reproducibility(m, n, pi, gpu_device):
    c = _case(m, n, pi)
    P, dev, sel = c["P"], c["xyz"].device, c["sel"].long()
    first = _run_capi(c)
    again = _run_capi(c)                                                 # bit-identical from run to run
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    out4, gx, gs, gr = first
    # accumulate = 0 on 0xFF-filled buffers: the selected rows are written, every other byte is as it was
    ff = [torch.full((P, w), -1, dtype=torch.int32, device=dev).view(torch.float32) for w in (3, 3, 4)]
    _, fx, fs, fr = _run_capi(c, fill=ff)
    outside = torch.ones(P, dtype=torch.bool, device=dev)
    outside[sel] = False
    for got, want in ((fx, gx), (fs, gs), (fr, gr)):
        assert bool((got.view(torch.int32)[outside] == -1).all())
        assert torch.equal(got[sel], want[sel])
    # accumulate = 1 on pre-filled buffers = pre-fill + the accumulate = 0 result on the selected rows
    gen = torch.Generator().manual_seed(9)
    pre = [torch.randn((P, w), generator=gen).to(dev) * 1e-3 for w in (3, 3, 4)]
    o4, ax, asc, ar = _run_capi(c, accumulate=True, fill=pre)
    assert torch.equal(o4, out4)
    for got, before, term in ((ax, pre[0], gx), (asc, pre[1], gs), (ar, pre[2], gr)):
        want = before.clone()
        want[sel] = before[sel] + term[sel]
        assert torch.equal(got, want)
    # nothing to do: {0, 0, 0, 0}, buffers untouched
    empty, ex, es, er = _run_capi(c, fill=ff, points=c["points"][:0])
    assert empty.tolist() == [0.0] * 4
    assert all(bool((g.view(torch.int32) == -1).all()) for g in (ex, es, er))
    huber, max_dist, lambda_flat = c["params"]
    none = _capi.surfel_plane_loss(c["points"], c["sel"][:0], c["xyz"], c["scaling"], c["rotation"], LAM, huber,
                                   max_dist, lambda_flat)
    assert none.tolist() == [0.0] * 4


@pytest.mark.parametrize("pi", range(3), ids=PIDS)
@pytest.mark.parametrize("m,n", [(65, 272), (2500, 16), (500, 8000)])
def test_the_order_of_the_points_moves_nothing_beyond_the_bar(m, n, pi, gpu_device):
    c = _case(m, n, pi)
    out4 = _run_capi(c)[0]
    perm = torch.randperm(c["m"], generator=torch.Generator().manual_seed(21)).to(c["xyz"].device)
    p4, px, ps, pr = _run_capi(c, points=c["points"][perm].contiguous())
    assert float(p4[3]) == float(out4[3])                      # an integer count over m: exact in any order
    assert torch.equal(p4[2], out4[2])                         # (the points do not enter the flatness prior)
    _check(c, p4, px, ps, pr, "permuted points")


@pytest.mark.parametrize("m,n", [(7, 16), (500, 8000)])
def test_terms_that_are_switched_off_leave_exact_zeros(m, n, gpu_device):
    c = _case(m, n, 1)
    huber, max_dist, lambda_flat = c["params"]
    out4, gx, gs, gr = _run_capi(c, params=(huber, max_dist, 0.0))
    assert not bool(gs.any()) and bool(gx.any()) and bool(gr.any())
    assert float(out4[0]) == float(torch.tensor(LAM) * out4[1].cpu())
    out4, gx, gs, gr = _run_capi(c, lam=0.0)
    assert not bool(gx.any()) and not bool(gr.any()) and bool(gs.any())
    assert float(out4[0]) == float(torch.tensor(lambda_flat) * out4[2].cpu()) and float(out4[1]) > 0
    ks = c["facts"]["ks"]
    rows = gs[c["sel"].long()]
    assert torch.equal(rows != 0, torch.nn.functional.one_hot(ks, 3).bool())      # the thin axis only
    assert bool((rows.sum(1) == float(torch.tensor(lambda_flat) / c["n"])).all())


def test_a_point_or_centre_that_is_not_finite_adds_nothing(gpu_device):
    c = _case(65, 272, 1)
    out4, gx, gs, gr = _run_capi(c)
    pts = torch.cat([c["points"], torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0]], device=c["xyz"].device)])
    o2, x2, s2, r2 = _run_capi(c, points=pts)
    m = c["m"]
    assert bool(torch.isfinite(o2).all()) and all(bool(torch.isfinite(g).all()) for g in (x2, s2, r2))
    assert round(float(o2[3]) * (m + 2)) == round(float(out4[3]) * m)              # neither passes the gate
    torch.testing.assert_close(o2[1] * (m + 2), out4[1] * m, rtol=4 * EPS32, atol=0)
    torch.testing.assert_close(x2 * (m + 2), gx * m, rtol=8 * EPS32, atol=0)
    # (an entry of J^T b is a difference of products that can cancel: absolute, against the largest entry)
    torch.testing.assert_close(r2 * (m + 2), gr * m, rtol=0, atol=16 * EPS32 * float((gr * m).abs().max()))


@pytest.mark.parametrize("off", [4, 8, 12])
def test_buffers_at_any_four_byte_offset(off, gpu_device):
    """Every array, the workspace included, as a view at `off` bytes inside a guarded allocation (tests/arena.py): the
    aligned run's bits, the guards intact."""
    c = _case(65, 272, 1)
    want = _run_capi(c)
    huber, max_dist, lambda_flat = c["params"]
    A = Arena(c["xyz"].device, offsets("a%d" % off))
    for k in ("points", "xyz", "scaling", "rotation"):
        A.put(k, c[k])
    A.put("sel", c["sel"].view(torch.float32))
    nbytes = int(G.lib().gsr_surfel_plane_loss_workspace(c["m"], c["n"]))
    A.put("ws", shape=((nbytes + 3) // 4,))
    A.put("out4", shape=(4,))
    for k, w in (("gx", 3), ("gs", 3), ("gr", 4)):
        A.put(k, torch.zeros((c["P"], w), device=c["xyz"].device))
    rc = G.lib().gsr_surfel_plane_loss(c["P"], c["m"], c["n"], A.ptr("points"), A.ptr("sel"), A.ptr("xyz"),
                                       A.ptr("scaling"), A.ptr("rotation"), LAM, huber, max_dist, lambda_flat,
                                       A.ptr("out4"), A.ptr("gx"), A.ptr("gs"), A.ptr("gr"), 0, A.ptr("ws"), nbytes,
                                       _capi._stream())
    assert rc == 0, G.lib().gsr_last_error()
    torch.cuda.synchronize()
    assert A.guards_intact() is None
    for k, w in zip(("out4", "gx", "gs", "gr"), want):
        assert torch.equal(A.t[k], w), k


@pytest.mark.parametrize("m,n,D", simi_ref.TIE_CASES)
def test_a_tie_goes_to_the_lowest_position_in_sel(m, n, D, gpu_device):
    """The similarity loss's tie rule is this term's (include/gsraster.h): tests/test_gpu_simi.py's test of this name
    has the inputs and the arithmetic of where the copies of a centre sit in the search (the two terms share the launch
    plan).  The copies of a centre carry other quaternions than the centre: a point that chose one would change the four
    outputs too.  lambda_flat = 0, max_dist = inf, and a dyadic knee that some residuals lie inside and some beyond."""
    c = simi_ref.tie_inputs(m, n, D, gpu_device)

    def run(sel):
        gx, gs, gr = (torch.zeros_like(c[k]) for k in ("xyz", "scaling", "rotation"))
        out4 = _capi.surfel_plane_loss(c["points"], sel, c["xyz"], c["scaling"], c["rotation"], LAM, 0.0625,
                                       float("inf"), 0.0, gx, gs, gr)
        return out4, gx, gr

    first, copies = c["sel"][:D].long(), c["sel"][D:].long()
    (out4, gx, gr), (want4, want_gx, want_gr) = run(c["sel"]), run(c["sel"][:D].contiguous())
    assert float(want4[3]) == 1.0 and float(want4[1]) > 0                  # every point is gated in and off its plane
    assert bool(want_gx[first].any(1).all())                               # every distinct centre is some point's nearest
    assert torch.equal(out4, want4)
    assert torch.equal(gx[first], want_gx[first]) and torch.equal(gr[first], want_gr[first])
    assert not bool(gx[copies].any()) and not bool(gr[copies].any())


def test_the_similarity_loss_keeps_its_bits(gpu_device):
    c = _case(500, 8000, 1)

    def simi():
        gx, gs = torch.zeros_like(c["xyz"]), torch.zeros_like(c["scaling"])
        out3 = _capi.similarity_loss(c["points"], c["sel"], c["xyz"], c["scaling"], LAM, gx, gs)
        return out3, gx, gs

    before = simi()
    _run_capi(c)
    after = simi()
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def _model_from(c, fused_tail):
    """GaussianParameters whose activated scales are the scene's (raw = log) and whose raw quaternions are the scene's
    times a positive factor, so that the activation's normalisation has a backward worth the name."""
    P, dev = c["P"], c["xyz"].device
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    stretch = (0.5 + torch.rand((P, 1), generator=gen)).to(dev)
    m = G.GaussianParameters(c["xyz"].clone(), r(P, 1, 3), r(P, 3, 3) * 0.1, c["scaling"].log(), c["rotation"] * stretch,
                             r(P, 1))
    m.fused_tail = fused_tail
    return m


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("m,n,pi", [(7, 16, 0), (500, 8000, 1)])
def test_autograd_node_on_both_activation_paths(m, n, pi, fused_tail, gpu_device):
    """The node's three gradients, scaled by the upstream 3, reach the leaves through FusedActivations' chain rule and
    are parked in `_act_grads` (rotation slot included) by the stashing tail: each equals the ctypes call chained by
    hand."""
    base = _case(m, n, pi)
    params = base["params"]
    model = _model_from(base, fused_tail)
    xyz, opac, scales, rot, shs = model.activated()
    c = dict(base)
    c["scaling"], c["rotation"] = scales.detach().clone(), rot.detach().clone()     # what the node sees
    a = PR.analyse(c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"], params)
    c["points"] = c["points"][~a["fragile"]].contiguous()
    assert c["points"].shape[0] >= 0.99 * base["m"]
    c = _with_refs(c, params)
    loss = G.surfel_plane_loss(c["points"], c["sel"], xyz, scales, rot, LAM, *params)
    parts = loss.grad_fn.parts
    assert loss.shape == () and float(parts[0]) == float(loss.detach()) and parts.shape == (4,)
    (3.0 * loss + 0.0 * (opac.sum() + shs.sum())).backward()
    out4, bx, bs, br = _run_capi(c)
    _check(c, parts, bx, bs, br, "autograd fused_tail=%d" % fused_tail)
    assert torch.equal(parts, out4)
    assert torch.equal(model._xyz.grad, bx * 3.0)
    if fused_tail:
        assert model._scaling.grad is None and model._rotation.grad is None        # parked, not chained
        assert torch.equal(model._act_grads[0], bs * 3.0) and torch.equal(model._act_grads[1], br * 3.0)
        assert not bool(model._act_grads[2].any()) and not bool(model._act_grads[3].any())
    else:
        want = _capi.activate_backward(model._rotation.detach().contiguous(), scales.detach(), opac.detach(), bs * 3.0,
                                       br * 3.0, torch.zeros_like(opac), torch.zeros_like(shs))
        assert torch.equal(model._scaling.grad, want[0]) and torch.equal(model._rotation.grad, want[1])
        sel = c["sel"].long()
        assert bool(model._rotation.grad[sel].any()) and bool(model._scaling.grad[sel].any()) == (params[2] > 0)
    # only the inputs that need a gradient get a buffer
    x = c["xyz"].clone().requires_grad_(True)
    only = G.surfel_plane_loss(c["points"], c["sel"], x, c["scaling"], c["rotation"], LAM, *params)
    assert only.grad_fn.grads[1] is None and only.grad_fn.grads[2] is None
    assert torch.equal(torch.autograd.grad(only, x)[0], bx)


def test_cpp_host_is_bit_identical_to_the_python_route(gpu_device):
    nx = G.torch_ops().next
    for m, n, pi in ((7, 16, 0), (65, 272, 2), (500, 8000, 1)):
        c = _case(m, n, pi)
        res = []
        for fn in (nx.surfel_plane_loss, G.surfel_plane_loss):
            x, s, q = (c[k].clone().requires_grad_(True) for k in ("xyz", "scaling", "rotation"))
            loss = fn(c["points"], c["sel"], x, s, q, LAM, *c["params"])
            res.append((loss.detach(),) + tuple(torch.autograd.grad(2.5 * loss, (x, s, q))))
        assert all(torch.equal(a, b) for a, b in zip(*res))
        out4, bx, bs, br = _run_capi(c)
        assert torch.equal(res[0][0], out4[0]) and torch.equal(res[0][3], br * 2.5) and torch.equal(res[0][1], bx * 2.5)
    with pytest.raises(ValueError):
        nx.surfel_plane_loss(c["points"], c["sel"].long(), c["xyz"], c["scaling"], c["rotation"], LAM)
    with pytest.raises(ValueError):
        nx.surfel_plane_loss(c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"][:, :3], LAM)


def test_calc_plane_loss_is_the_explicit_call_on_calc_simi_loss_selection(gpu_device):
    c = _case(500, 8000, 1)
    sc, P, dev = c["scene"], c["P"], c["xyz"].device
    huber, max_dist, lambda_flat = c["params"]
    kw = dict(huber=huber, max_dist=max_dist, lambda_flat=lambda_flat)
    models = []
    for with_index in (True, False):
        model = G.GrowableGaussians(1024, 1, dev)
        G.GrowableAdam(model)
        rgbs = (torch.rand((P, 3), generator=torch.Generator().manual_seed(4)) * 255).to(dev)
        idx = dict(voxel_keys=sc["keys"], voxel_counts=sc["counts"]) if with_index else {}
        assert model.add_new_pointcloud(c["xyz"], torch.diag_embed(c["scaling"] ** 2), rgbs, 1.0, **idx) == (0, P)
        models.append(model)
    model, bare = models
    assert bare.calc_plane_loss(sc["losses"], LAM, **kw) is None and bare.calc_simi_loss(sc["losses"], LAM) is None
    assert model.calc_plane_loss({123456789: torch.zeros(2, 3)}, LAM, **kw) is None
    for fused_tail in (False, True):
        model.fused_tail = fused_tail
        xyz, opac, scales, rot, shs = model.activated()
        points, sel = model.voxel_index.select(sc["losses"], max_points=10 ** 9)
        assert torch.equal(sel, c["sel"])
        whole = model.calc_plane_loss(sc["losses"], LAM, scaling=scales, rotation=rot, max_points=10 ** 9, **kw)
        explicit = G.surfel_plane_loss(points, sel, model._xyz, scales, rot, LAM, huber, max_dist, lambda_flat)
        assert whole.shape == () and float(whole.detach()) == float(explicit.detach()) > 0
        assert torch.equal(whole.grad_fn.parts, explicit.grad_fn.parts)
        gen = lambda: torch.Generator().manual_seed(6)  # noqa: E731
        cut = model.calc_plane_loss(sc["losses"], LAM, scaling=scales, rotation=rot, generator=gen(), **kw)
        pts500, sel500 = model.voxel_index.select(sc["losses"], generator=gen())
        assert pts500.shape == (500, 3)
        assert float(cut) == float(G.surfel_plane_loss(pts500, sel500, model._xyz, scales, rot, LAM, **kw))
        (whole + 0.0 * (opac.sum() + shs.sum())).backward()
        assert bool(model._xyz.grad.any())
        model._xyz.grad = None
        model._act_grads = None
    getter = model.calc_plane_loss(sc["losses"], LAM, max_points=10 ** 9, **kw)          # the getter route
    assert float(getter) == float(explicit)


# mutant -> the named checks of which at least one must refuse it, at (500, 8000) with huber 0.02, max_dist 0.05,
# lambda_flat 0.3 (a mutant of a gradient line leaves the four outputs alone)
REFUSED_BY = {"largest_scale_column": ("mean_rho", "mean_thin", "gx", "gs", "gr"), "transposed_R": ("mean_rho", "gx", "gr"),
              "sign_dropped_from_B": ("gr",), "gate_on_d2": ("gate_share",), "huber_slope_halved": ("gx",),
              "w_gradient_dropped": ("gr",)}


def test_every_mutant_of_the_restatement_is_refused_by_a_named_check(gpu_device):
    c = _case(500, 8000, 1)
    args = (c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"])
    good = PR.plane_loss_closed(*args, c["params"])                       # float32 arithmetic, no mutant: passes
    rec = _compare(c, good["out4"], good["gx"], good["gs"], good["gr"])
    assert all(rec[k]["ratio"] <= 1.0 for k in QUANTITIES), rec
    assert set(REFUSED_BY) == set(PR.MUTANTS)
    for mutant, named in REFUSED_BY.items():
        w = PR.plane_loss_closed(*args, c["params"], mutant=mutant)
        rec = _compare(c, w["out4"], w["gx"], w["gs"], w["gr"])
        refused = [k for k in QUANTITIES if rec[k]["ratio"] > 1.0]
        print(json.dumps(dict(mutant=mutant, refused_by={k: rec[k]["ratio"] for k in refused})))
        assert all(k in refused for k in named), (mutant, refused)
        if mutant in ("sign_dropped_from_B", "huber_slope_halved", "w_gradient_dropped"):
            assert not any(k in refused for k in QUANTITIES[:4]), (mutant, refused)
