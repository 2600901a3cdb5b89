"""GPU tests of the fused LiDAR similarity loss (csrc/simi.hip, gsr_similarity_loss; loss.py, model.py, torch_next.cpp)
against the float64 restatement of GaussianModel::compute_min_distance (tests/simi_ref.py).

How close is close enough (no constant is picked).  The yardstick is the reference's own arithmetic: the same
restatement run in float32 Torch ops on the same inputs.  Its distance e_ref to the float64 result is measured per
quantity -- loss, r, every selected row of the xyz gradient, the scale-gradient value -- and the HIP result may be

    max(2 * e_ref, K * eps32 * magnitude)

away from float64.  The factor 2: our reduction order is not Torch's, so we may err by as much as Torch in the other
direction.  K * eps32 * magnitude is the floor where Torch happens to be exact (e_ref = 0, usual for m = 1): K counts
the float32 roundings between the inputs and a result, one eps32 = 2^-23 each (twice the unit roundoff: headroom for
the error of d entering 1/d): three subtractions (p - x), three multiply-adds (the squared norm), one square root,
one subtraction of r, one division ((p - x)/d, or the mean's division) = 9, plus the depth of a pairwise reduction
over the longer of the two sums (3n scale elements, m points), ceil(log2(max(3n, m))).  The magnitude is what those
relative errors scale with, taken in float64: d + r for a clamped distance d - r (the absolute errors of d and of r
both enter), so lambda * mean_i(d_i + r) for the loss and r for r; lambda/m times the number of points that share the
row for a row of the xyz gradient (each point adds a vector of length lambda/m); the value itself for the scale
gradient.

Fragile points.  A point whose two nearest selected Gaussians differ in distance by less than 1e-5 relative, or
whose |d - r| < 1e-5 (d + r), may choose the other row or the other side of the clamp in float32: it is removed from
the inputs of BOTH sides (the float64 result is recomputed without it, no row is masked), and a case fails if that
removes more than 1 % of its points.  Figures measured on an MI355X are recorded in DESIGN.md section 2.
"""
import functools
import json
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import simi_ref as R
from gs_livm_amd import _capi

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
LAM = 0.2
# (m, n) -> how the scene maker gets there: selected voxels, Gaussians per voxel
# (the issue's five sizes, and 2 500 points in ONE voxel: every Gaussian is the nearest of ~150 points, whose records
# lie in several staging tiles of the gradient pass)
CASES = {(1, 1): (1, 1), (7, 16): (1, 16), (500, 8000): (500, 16), (500, 32000): (2000, 16), (3000, 50000): (3125, 16),
         (2500, 16): (1, 16)}
LARGE = [(500, 8000), (500, 32000), (3000, 50000)]


def _analyse(points, sel, xyz, scaling):
    """float64: nearest distance and its position in sel per point, r, and which points are fragile.  Plain
    broadcasting in blocks of points (no cdist / topk: nothing here should depend on a library's choice of
    algorithm at a given size)."""
    x = xyz.double().index_select(0, sel.long())
    r = scaling.double().index_select(0, sel.long()).mean()
    p = points.double()
    d1, d2, arg = [], [], []
    for lo in range(0, p.shape[0], 256):
        d = (p[lo:lo + 256, None, :] - x[None, :, :]).norm(2, 2)
        best, idx = d.min(1)
        d1.append(best)
        arg.append(idx)
        if d.shape[1] > 1:
            d.scatter_(1, idx[:, None], float("inf"))
            d2.append(d.min(1).values)
    d1, arg = torch.cat(d1), torch.cat(arg)
    fragile = (d1 - r).abs() < 1e-5 * (d1 + r)
    if d2:
        fragile |= (torch.cat(d2) - d1) < 1e-5 * d1
    return d1, arg, r, fragile


def _reference(points, sel, xyz, scaling, dtype):
    x = xyz.to(dtype).requires_grad_(True)
    s = scaling.to(dtype).requires_grad_(True)
    loss = R.similarity_loss_ref(points.to(dtype), sel, x, s, LAM)
    gx, gs = torch.autograd.grad(loss, (x, s))
    r = s.detach().index_select(0, sel.long()).mean()
    return dict(loss=loss.detach().double(), r=r.double(), gx=gx.double(), gs=gs.double())


@functools.lru_cache(maxsize=None)
def _case(m, n):
    dev = torch.device("cuda:0")
    voxels, per = CASES[(m, n)]
    sc = R.make_scene(voxels, m, seed=1000 + n + m, per_voxel=per, empty_voxels=0 if voxels == 1 else 3)
    vi = G.VoxelIndex(dev)
    vi.add(sc["keys"], sc["counts"], 0)
    points, sel = vi.select(sc["losses"], max_points=10 ** 9)
    assert points.shape == (m, 3) and sel.shape == (n,) and sc["P"] >= (4 * n if n > 16 else n)
    xyz, scaling = torch.from_numpy(sc["xyz"]).to(dev), torch.from_numpy(sc["scaling"]).to(dev)
    _, _, _, fragile = _analyse(points, sel, xyz, scaling)
    removed = int(fragile.sum())
    assert removed <= 0.01 * m, "%d of %d points are fragile" % (removed, m)
    points = points[~fragile].contiguous()
    d1, arg, r, fragile = _analyse(points, sel, xyz, scaling)
    assert not bool(fragile.any())
    ref64 = _reference(points, sel, xyz, scaling, torch.float64)
    ref32 = _reference(points, sel, xyz, scaling, torch.float32)
    mm = points.shape[0]
    active = d1 > r
    shares = torch.bincount(arg[active], minlength=n).double()          # points per selected row, float64 argmin
    K = 9 + math.ceil(math.log2(max(3 * n, mm)))
    return dict(points=points, sel=sel, xyz=xyz, scaling=scaling, P=sc["P"], m=mm, n=n, removed=removed, d1=d1, r=r,
                inside=int((~active).sum()), shares=shares, K=K, ref64=ref64, ref32=ref32, scene=sc)


def _bars(c):
    """Per quantity: (e_ref, bar) as the module docstring derives them."""
    a, b, K, sel = c["ref64"], c["ref32"], c["K"], c["sel"].long()
    out = {}
    e = float((b["loss"] - a["loss"]).abs())
    out["loss"] = (e, max(2 * e, K * EPS32 * LAM * float((c["d1"] + c["r"]).mean())))
    e = float((b["r"] - a["r"]).abs())
    out["r"] = (e, max(2 * e, K * EPS32 * float(c["r"])))
    e_rows = (b["gx"] - a["gx"]).index_select(0, sel).abs().amax(1)
    out["gx"] = (e_rows, torch.maximum(2 * e_rows, K * EPS32 * (LAM / c["m"]) * c["shares"]))
    e = float((b["gs"] - a["gs"]).index_select(0, sel).abs().max())
    out["gs"] = (e, max(2 * e, K * EPS32 * float(a["gs"].index_select(0, sel).abs().max())))
    return out


def _run_capi(c, accumulate=False, fill=None):
    P, dev = c["P"], c["xyz"].device
    if fill is None:
        gx, gs = torch.zeros((P, 3), device=dev), torch.zeros((P, 3), device=dev)
    else:
        gx, gs = fill[0].clone(), fill[1].clone()
    out3 = _capi.similarity_loss(c["points"], c["sel"], c["xyz"], c["scaling"], LAM, gx, gs, accumulate=accumulate)
    return out3, gx, gs


def _check(c, loss, r, gx, gs, what):
    """Holds one HIP result (gx / gs dense [P,3]) against float64 at the derived bars; prints every figure first."""
    a, bars, sel = c["ref64"], _bars(c), c["sel"].long()
    err = {"loss": float((loss.double() - a["loss"]).abs())}
    if r is not None:
        err["r"] = float((r.double() - a["r"]).abs())
    rows = (gx.double() - a["gx"]).index_select(0, sel).abs().amax(1)
    err["gs"] = float((gs.double() - a["gs"]).index_select(0, sel).abs().max())
    worst = float((rows / bars["gx"][1].clamp(min=1e-300)).max()) if bool((bars["gx"][1] > 0).any()) else 0.0
    print(json.dumps(dict(what=what, m=c["m"], n=c["n"], P=c["P"], removed=c["removed"], inside_r=c["inside"], K=c["K"],
                          loss=float(a["loss"]), loss_e_ref=bars["loss"][0], loss_bar=bars["loss"][1], loss_err=err["loss"],
                          r_e_ref=bars["r"][0], r_bar=bars["r"][1], r_err=err.get("r"),
                          gx_e_ref_max=float(bars["gx"][0].max()), gx_err_max=float(rows.max()), gx_worst_over_bar=worst,
                          gs_e_ref=bars["gs"][0], gs_bar=bars["gs"][1], gs_err=err["gs"])))
    assert err["loss"] <= bars["loss"][1]
    if r is not None:
        assert err["r"] <= bars["r"][1]
    assert bool((rows <= bars["gx"][1]).all()), "xyz gradient: worst row at %.3g of its bar" % worst
    assert err["gs"] <= bars["gs"][1]
    outside = torch.ones(c["P"], dtype=torch.bool, device=gx.device)
    outside[sel] = False
    assert not bool(gx[outside].any()) and not bool(gs[outside].any())   # rows outside the selection: exactly zero


@pytest.mark.parametrize("m,n", list(CASES))
def test_capi_matches_float64_at_the_derived_bar(m, n, gpu_device):
    c = _case(m, n)
    out3, gx, gs = _run_capi(c)
    assert float(out3[0]) == np.float32(LAM) * np.float32(float(out3[1]))   # {loss, loss before lambda, r}
    _check(c, out3[0], out3[2], gx, gs, "capi")
    # forward only: the same three numbers, no gradient buffer needed
    only = _capi.similarity_loss(c["points"], c["sel"], c["xyz"], c["scaling"], LAM)
    assert torch.equal(only, out3)


@pytest.mark.parametrize("m,n", LARGE)
def test_both_branches_of_the_clamp_are_exercised(m, n, gpu_device):
    c = _case(m, n)
    assert 0.02 * c["m"] <= c["inside"] <= 0.5 * c["m"], (c["inside"], c["m"])


def test_many_points_share_a_nearest_gaussian(gpu_device):
    """The many-to-one accumulation of the xyz gradient, at the same bar (test_capi_... runs the case too)."""
    c = _case(2500, 16)
    assert float(c["shares"].max()) >= 50 and float(c["shares"].sum()) == c["m"] - c["inside"]
    out3, gx, gs = _run_capi(c)
    _check(c, out3[0], out3[2], gx, gs, "shared rows")


@pytest.mark.parametrize("m,n", [(7, 16), (500, 8000), (3000, 50000)])
def test_accumulate_untouched_rows_and_reproducibility(m, n, gpu_device):
    c = _case(m, n)
    P, dev, sel = c["P"], gpu_device, c["sel"].long()
    out3, gx, gs = _run_capi(c)
    for _ in range(2):                                                   # bit-identical from run to run
        o2, gx2, gs2 = _run_capi(c)
        assert torch.equal(o2, out3) and torch.equal(gx2, gx) and torch.equal(gs2, gs)
    # accumulate = 0 on 0xFF-filled buffers: the selected rows are written, every other byte is as it was
    ff = torch.full((P, 3), float("nan"), device=dev).view(torch.int32).fill_(-1).view(torch.float32)
    _, fx, fs = _run_capi(c, fill=(ff, ff))
    outside = torch.ones(P, dtype=torch.bool, device=dev)
    outside[sel] = False
    for got, want in ((fx, gx), (fs, gs)):
        assert bool((got.view(torch.int32)[outside] == -1).all())
        assert torch.equal(got[sel], want[sel])
    # accumulate = 1 on pre-filled buffers = pre-fill + the accumulate = 0 result on the selected rows
    gen = torch.Generator().manual_seed(9)
    pre = (torch.randn((P, 3), generator=gen).to(dev) * 1e-3, torch.randn((P, 3), generator=gen).to(dev) * 1e-3)
    o3, ax, asc = _run_capi(c, accumulate=True, fill=pre)
    assert torch.equal(o3, out3)
    for got, before, term in ((ax, pre[0], gx), (asc, pre[1], gs)):
        want = before.clone()
        want[sel] = before[sel] + term[sel]
        assert torch.equal(got, want)
    # nothing to do: {0, 0, 0}, buffers untouched
    empty = _capi.similarity_loss(c["points"][:0], c["sel"], c["xyz"], c["scaling"], LAM, fx, fs)
    assert empty.tolist() == [0.0, 0.0, 0.0] and bool((fx.view(torch.int32)[outside] == -1).all())
    assert _capi.similarity_loss(c["points"], c["sel"][:0], c["xyz"], c["scaling"], LAM).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("m,n,D", R.TIE_CASES)
def test_a_tie_goes_to_the_lowest_position_in_sel(m, n, D, gpu_device):
    """Of several selected centres at bit-equal squared distance the lowest position in `sel` wins (include/gsraster.h),
    whichever wave, tile or chunk of the search holds the others.  R.tie_inputs: position k holds lattice point k mod D,
    exact in float32, so the call on the whole selection must give the bits of the call on its first D positions, and
    no copy (position >= D) may receive a gradient.  Where the copies sit, by the launch plan's arithmetic (64 points
    per point block, 256 centres per tile, a quarter of a tile per wave, chunks = min(1024 // point blocks, tiles)):
      m = 64, n = 768, D = 64:      1 point block, 3 tiles, min(1024, 3) = 3 chunks of 1 tile.  Centre j has copies at
          j + 64, j + 128, j + 192 (the other three waves of its tile) and at j + 256 .. j + 704 (the other two chunks).
      m = 32768, n = 768, D = 192:  512 point blocks, 3 tiles, 1024 // 512 = 2 chunks of ceil(3 / 2) = 2 tiles: chunk 0
          is tiles 0-1, chunk 1 is tile 2.  For j < 64, position 64 + j (tile 0, wave 1) ties with 256 + j (tile 1,
          wave 0): wave 0 scans positions 0 .. 63 and then 256 .. 319, so it holds the LATER position of the two and
          the combine of the four waves must settle it by the position.  Positions j and 128 + j tie with 576 + j and
          512 + j, which lie in chunk 1."""
    c = R.tie_inputs(m, n, D, gpu_device)

    def run(sel):
        gx, gs = torch.zeros_like(c["xyz"]), torch.zeros_like(c["scaling"])
        return _capi.similarity_loss(c["points"], sel, c["xyz"], c["scaling"], LAM, gx, gs), gx

    first, copies = c["sel"][:D].long(), c["sel"][D:].long()
    (out3, gx), (want3, want_gx) = run(c["sel"]), run(c["sel"][:D].contiguous())
    assert float(want3[2]) == 2.0 ** -6 and float(want3[1]) > 0.1          # r, and every point far outside it
    assert bool(want_gx[first].any(1).all())                               # every distinct centre is some point's nearest
    assert torch.equal(out3, want3)
    assert torch.equal(gx[first], want_gx[first])
    assert not bool(gx[copies].any())


def _model_from(c, fused_tail):
    """GaussianParameters whose activated scales are the scene's (raw = log) -- exp(log(s)) rounds: the float64
    reference is taken at the activated values the node actually saw."""
    P, dev = c["P"], c["xyz"].device
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    m = G.GaussianParameters(c["xyz"].clone(), r(P, 1, 3), r(P, 3, 3) * 0.1, c["scaling"].log(), r(P, 4), r(P, 1))
    m.fused_tail = fused_tail
    return m


@pytest.mark.parametrize("fused_tail", [False, True])
@pytest.mark.parametrize("m,n", [(7, 16), (500, 8000)])
def test_autograd_node_on_both_activation_paths(m, n, fused_tail, gpu_device):
    """The node's gradients reach the leaves through FusedActivations' chain rule, and through the stashing tail they
    are ADDED to what another consumer of the activated scales (here a stand-in for the rasterizer) parks."""
    c = dict(_case(m, n))
    model = _model_from(c, fused_tail)
    xyz, opac, scales, rot, shs = model.activated()
    c["scaling"] = scales.detach().clone()       # what the node sees
    c["ref64"] = _reference(c["points"], c["sel"], c["xyz"], c["scaling"], torch.float64)
    c["ref32"] = _reference(c["points"], c["sel"], c["xyz"], c["scaling"], torch.float32)
    c["r"] = c["ref64"]["r"]
    loss = G.similarity_loss(c["points"], c["sel"], xyz, scales, LAM)
    parts = loss.grad_fn.parts
    assert loss.shape == () and float(parts[0]) == float(loss)
    other = torch.full_like(scales, 0.25)        # a second consumer: d/dscales of 0.25 * sum(scales)
    (3.0 * loss + 0.25 * scales.sum() + 0.0 * (rot.sum() + opac.sum() + shs.sum())).backward()
    if fused_tail:
        g_act = model._act_grads[0]
        assert model._scaling.grad is None       # parked, not chained
    else:
        g_act = model._scaling.grad / scales.detach()    # d exp(s)/ds = exp(s)
    gs = (g_act - other) / 3.0
    gx = model._xyz.grad / 3.0
    # the detour through (x3, +0.25, -0.25, /3[, * and / by exp]) rounds a few more times than the bare call:
    # compare the bare ctypes result at the bar, and this route to the bare result within those roundings
    out3, bx, bs = _run_capi(c)
    _check(c, loss.detach(), parts[2], bx, bs, "autograd fused_tail=%d" % fused_tail)
    assert float(out3[0]) == float(loss)
    torch.testing.assert_close(gx, bx, rtol=4 * EPS32, atol=0)
    sel = c["sel"].long()
    torch.testing.assert_close(gs[sel], bs[sel], rtol=0, atol=8 * EPS32 * 0.25)   # (cancellation against 0.25)
    if fused_tail:
        torch.testing.assert_close(g_act, other + 3.0 * bs, rtol=2 * EPS32, atol=0)


def test_cpp_host_is_bit_identical_to_the_python_route(gpu_device):
    nx = G.torch_ops().next
    for m, n in ((7, 16), (500, 8000)):
        c = _case(m, n)
        res = []
        for fn in (nx.similarity_loss, G.similarity_loss):
            x = c["xyz"].clone().requires_grad_(True)
            s = c["scaling"].clone().requires_grad_(True)
            loss = fn(c["points"], c["sel"], x, s, LAM)
            gx, gs = torch.autograd.grad(2.5 * loss, (x, s))
            res.append((loss.detach(), gx, gs))
        assert all(torch.equal(a, b) for a, b in zip(*res))
        # the selection: same rows, same points
        sc = c["scene"]
        vi_c, vi_p = nx.VoxelIndex(), G.VoxelIndex(gpu_device)
        assert vi_c.add(sc["keys"], sc["counts"], 0) == vi_p.add(sc["keys"], sc["counts"], 0) == c["P"]
        assert len(vi_c) == len(vi_p) and sc["keys"][0] in vi_c
        pc, sel_c = vi_c.select(sc["losses"], 10 ** 9, "cuda")
        pp, sel_p = vi_p.select(sc["losses"], max_points=10 ** 9)
        assert sel_c.dtype == torch.int32 and torch.equal(sel_c, sel_p) and torch.equal(pc, pp)
        if m >= 500:   # the cut to exactly 500: the same draw from the default generator on both routes
            torch.manual_seed(11)
            pc, _ = vi_c.select(sc["losses"], 500, "cuda")
            torch.manual_seed(11)
            pp, _ = vi_p.select(sc["losses"], max_points=500)
            assert pc.shape == (500, 3) and torch.equal(pc, pp)
        with pytest.raises(ValueError):
            vi_c.add([sc["keys"][0]], [1], c["P"])
        assert vi_c.select({123456789: torch.zeros(2, 3)}, 500, "cuda") is None
    with pytest.raises(ValueError):
        nx.similarity_loss(c["points"], c["sel"].long(), c["xyz"], c["scaling"], LAM)


def _grown_model(c, dev, with_index=True):
    """GrowableGaussians grown by the scene's cloud in two events; covariances whose diagonal is scale^2."""
    sc = c["scene"]
    P = c["P"]
    model = G.GrowableGaussians(1024, 1, dev)
    opt = G.GrowableAdam(model)
    covs = torch.diag_embed(c["scaling"] ** 2)
    gen = torch.Generator().manual_seed(4)
    rgbs = (torch.rand((P, 3), generator=gen) * 255).to(dev)
    cut_v = len(sc["keys"]) // 2
    cut = int(sum(sc["counts"][:cut_v]))
    for lo, hi, kv in ((0, cut, slice(0, cut_v)), (cut, P, slice(cut_v, None))):
        kw = dict(voxel_keys=sc["keys"][kv], voxel_counts=sc["counts"][kv]) if with_index else {}
        assert model.add_new_pointcloud(c["xyz"][lo:hi], covs[lo:hi], rgbs[lo:hi], 1.0, **kw) == (lo, hi)
    model.fused_tail = True
    return model, opt


def test_one_optimiser_step_moves_the_parameters_like_the_torch_term(gpu_device):
    """render + photometric loss + similarity term + GrowableAdam.step_model, with the term from the HIP node (A) and
    written in Torch float32 ops (B); C carries no term and gives the photometric gradient alone.

    Gradients that reach the optimiser: expected = C's gradient + the term's float64 gradient; A may be
    max(2 * |B - expected|, K eps32 magnitude) + eps32 |expected| away (the module docstring's bar; the last summand
    is the one float32 addition that joins the two terms, made on both sides).
    Parameters: the first Adam step moves an element by lr * g / (|g| + 1e-15), i.e. by lr * sign(g) whatever the size
    of g, so where the gradient is distinguishable from zero (|expected| above its bar) A and B may differ by the
    roundings of that arithmetic only, 8 eps32 lr + eps32 |p|; elsewhere by at most the 2 lr of an undetermined
    sign."""
    dev = gpu_device
    c = dict(_case(500, 8000))
    W, H = 160, 120
    cam = G.Camera(torch.eye(3), (0.0, 0.0, -4.0), math.radians(60.0), 2.0 * math.atan(math.tan(math.radians(30.0)) * H / W),
                   W, H, device=dev)
    gt = torch.rand((3, H, W), generator=torch.Generator().manual_seed(8)).to(dev)
    bg = torch.zeros(3, device=dev)
    runs = {}
    for name in "ABC":
        model, opt = _grown_model(c, dev)
        names = ("_xyz", "_scaling")
        before = {k: getattr(model, k).detach().clone() for k in names}
        img = G.render(cam, model, bg)[0]
        loss = G.photometric_loss(img, gt, 0.2)
        scales = model.Get_scaling()
        if name == "A":
            picked = model.voxel_index.select(c["scene"]["losses"], max_points=10 ** 9)
            assert torch.equal(picked[1], c["sel"])
            term = G.similarity_loss(c["points"], c["sel"], model._xyz, scales, LAM)   # (the fragile-free points)
            whole = model.calc_simi_loss(c["scene"]["losses"], LAM, scaling=scales, max_points=10 ** 9)
            if c["removed"] == 0:
                assert float(whole) == float(term)
            loss = loss + term
        elif name == "B":
            loss = loss + R.similarity_loss_ref(c["points"], c["sel"], model._xyz, scales, LAM)
        loss.backward()
        grads = dict(_xyz=model._xyz.grad.clone(), _scaling=model._act_grads[0].clone())
        act_scales = scales.detach().clone()
        opt.step_model(model)
        runs[name] = dict(grads=grads, before=before, after={k: getattr(model, k).detach().clone() for k in names},
                          scales=act_scales, lr={"_xyz": opt.param_groups[0]["lr"], "_scaling": opt.param_groups[3]["lr"]})
    assert torch.equal(runs["A"]["scales"], runs["B"]["scales"])
    assert bool(runs["C"]["grads"]["_xyz"].any())                        # the render does reach the model
    c["scaling"] = runs["A"]["scales"]
    c["xyz"] = runs["A"]["before"]["_xyz"]
    c["ref64"] = _reference(c["points"], c["sel"], c["xyz"], c["scaling"], torch.float64)
    c["ref32"] = _reference(c["points"], c["sel"], c["xyz"], c["scaling"], torch.float32)
    c["r"] = c["ref64"]["r"]
    K, sel = c["K"], c["sel"].long()
    mag = {"_xyz": torch.zeros(c["P"], dtype=torch.float64, device=dev),
           "_scaling": torch.zeros(c["P"], dtype=torch.float64, device=dev)}
    mag["_xyz"][sel] = (LAM / c["m"]) * c["shares"]
    mag["_scaling"][sel] = float(c["ref64"]["gs"].index_select(0, sel).abs().max())
    for k, term64 in (("_xyz", c["ref64"]["gx"]), ("_scaling", c["ref64"]["gs"])):
        expected = runs["C"]["grads"][k].double() + term64
        e_ref = (runs["B"]["grads"][k].double() - expected).abs()
        err = (runs["A"]["grads"][k].double() - expected).abs()
        bar = torch.maximum(2 * e_ref, K * EPS32 * mag[k][:, None]) + EPS32 * expected.abs()
        print(json.dumps(dict(what="loop step gradient " + k, e_ref_max=float(e_ref.max()), err_max=float(err.max()),
                              worst_over_bar=float((err / bar.clamp(min=1e-300))[bar > 0].max()))))
        assert bool((err <= bar).all())
        lr = runs["A"]["lr"][k]
        pa, pb = runs["A"]["after"][k].double(), runs["B"]["after"][k].double()
        sure = expected.abs() > bar
        tol = torch.where(sure, torch.full_like(bar, 8 * EPS32 * lr), torch.full_like(bar, 2 * lr * (1 + 8 * EPS32)))
        tol = tol + EPS32 * pa.abs()
        moved = (runs["A"]["after"][k] != runs["A"]["before"][k])
        print(json.dumps(dict(what="loop step parameters " + k, moved=int(moved.sum()), sure=int(sure.sum()),
                              diff_max=float((pa - pb).abs().max()), lr=lr)))
        assert bool(((pa - pb).abs() <= tol).all())
        assert bool(moved[sel].any())
    # and the term does move the selected rows: without it (C) the step differs
    assert not torch.equal(runs["A"]["after"]["_xyz"][sel], runs["C"]["after"]["_xyz"][sel])


def test_growth_rows_do_not_depend_on_the_index_arguments(gpu_device):
    c = _case(500, 8000)
    a, _ = _grown_model(c, gpu_device, with_index=True)
    b, _ = _grown_model(c, gpu_device, with_index=False)
    for k in G.GrowableGaussians._NAMES:
        assert torch.equal(getattr(a, k).detach(), getattr(b, k).detach()), k
    assert len(b.voxel_index) == 0 and len(a.voxel_index) == len(c["scene"]["keys"])
    assert b.calc_simi_loss(c["scene"]["losses"], LAM) is None
    loss = a.calc_simi_loss(c["scene"]["losses"], LAM)                 # the getter route, subsampled to 500
    assert loss.shape == () and float(loss) > 0
