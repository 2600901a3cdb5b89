"""GPU tests of the fused delta-depth loss (csrc/delta.hip, gsr_delta_depth_loss; loss.py, torch_next.cpp).

Against float64: `warped`, out3 = {L, mean gap, mask share}, dL/ddepth_src and dL/ddepth_ref of every case of
tests/delta_ref.py (shapes 2x2, 5x3, 37x61, 64x80, 70x130 -- workgroup seams on both axes -- and 512x640 once, where the
finalize walks the 1280 partial sums in more than one pass; four poses; holes, clamped ref depths, masks on both sides),
each held per pixel to max(2 e_ref, bar) with the bars counted from the kernels' arithmetic in delta_ref.py's docstring
(K = 6 roundings per composed dot product and fma, the first-order term of the coordinate rounding through the bilinear
slopes, the fixed-point term N_j N Mx 2^-59 of the integer accumulation), fragile pixels removed from both sides and
capped at 1 %.  tests/test_delta_ref.py checks on the CPU that the float32 restatement stays inside the same bars.
Every case prints its worst |error| / bar; DESIGN.md section 2, "Delta-depth loss", is where they are recorded.

Exact properties: reproducibility bit for bit, NaN-prefilled outputs fully written, null gradients leave out3 and warped
unchanged, doubling lambda doubles L and both gradients exactly, an all-masked pair gives {0, 0, 0} and zero gradients,
every tensor and the workspace at 0/4/8/12 bytes inside guarded allocations (tests/arena.py), a refusal writes nothing,
one +Inf depth is "outside", and the Python autograd, ctypes and C++ routes agree bit for bit.  The loop test feeds two
rendered views to the term and follows the gradient into the rasterizer's backward."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import delta_ref as D
import gs_livm_amd as G
from arena import Arena, offsets
from gs_livm_amd import synthetic as S

pytestmark = pytest.mark.gpu
F64 = torch.float64
IMAGES = ("depth_src", "acc_src", "depth_ref", "acc_ref")


def _mat(a, n):
    return (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:n]])


def _call(dev, x, lam=None, mode="a0", warped=True, g_src=True, g_ref=True, short=0):
    """gsr_delta_depth_loss through ctypes with every device tensor and the workspace (exactly the queried size) inside
    guarded allocations; returns ({name: tensor copy}, arena, return code)."""
    L = G.lib()
    H, W = x["H"], x["W"]
    ar = Arena(dev, offsets(mode))
    for k in IMAGES:
        ar.put(k, torch.from_numpy(x[k]).to(dev))
    ar.put("out3", shape=(3,))
    for k, want in (("warped", warped), ("g_src", g_src), ("g_ref", g_ref)):
        if want:
            ar.put(k, shape=(H, W))
    nbytes = int(L.gsr_delta_depth_loss_workspace(H, W))
    assert nbytes % 4 == 0
    ar.put("ws", shape=(nbytes // 4,))
    p = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t else None  # noqa: E731
    rc = L.gsr_delta_depth_loss(H, W, p("depth_src"), p("acc_src"), p("depth_ref"), p("acc_ref"), _mat(x["inv_K_src"], 9),
                                _mat(x["K_ref"], 9), _mat(x["T_rel"], 12), float(x["lam"] if lam is None else lam),
                                p("out3"), p("warped"), p("g_src"), p("g_ref"), p("ws"), nbytes - short,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = {k: ar.t[k].clone() for k in ("out3", "warped", "g_src", "g_ref") if k in ar.t}
    return out, ar, rc


def _as_ref(o):
    return dict(warped=o["warped"].cpu().to(F64), grad_src=o["g_src"].cpu().to(F64), grad_ref=o["g_ref"].cpu().to(F64),
                loss=float(o["out3"][0]), mean_gap=float(o["out3"][1]), share=float(o["out3"][2]))


@pytest.mark.parametrize("case", D.CASE_NAMES)
def test_matches_float64(case, gpu_device):
    x, ref = D.inputs(case), D.reference(case)
    o, ar, rc = _call(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    for k in ("out3", "warped", "g_src", "g_ref"):
        assert not torch.isnan(o[k]).any(), k
    r = D.ratios(_as_ref(o), ref)
    print(case, "fragile share %.4f" % ref["fragile_share"], "worst |d| / bar:", {k: round(v, 3) for k, v in r.items()})
    assert ref["fragile_share"] <= 0.01
    assert max(r.values()) <= 1.0, r
    if x["H"] * x["W"] > 100:
        assert o["g_src"].any() and o["g_ref"].any() and float(o["out3"][0]) > 0


@pytest.mark.parametrize("case", ["5x3", "37x61_rpy", "64x80_shift", "70x130_rpy", "70x130_backward"])
def test_exact_properties(case, gpu_device):
    dev, x = gpu_device, D.inputs(case)
    a, ar, rc = _call(dev, x)
    assert rc == 0 and ar.guards_intact() is None
    b, _, _ = _call(dev, x)
    for k in a:                                       # reproducible; written in full over the NaN prefill
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert not torch.isnan(a[k]).any(), k
    # null gradients (each alone and both): out3 and warped bit for bit, the other gradient too
    for gs, gr in ((False, False), (True, False), (False, True)):
        n, ar2, rc = _call(dev, x, g_src=gs, g_ref=gr)
        assert rc == 0 and ar2.guards_intact() is None
        for k in n:
            assert torch.equal(n[k].view(torch.int32), a[k].view(torch.int32)), (k, gs, gr)
    n, _, rc = _call(dev, x, warped=False)
    assert rc == 0
    for k in n:
        assert torch.equal(n[k].view(torch.int32), a[k].view(torch.int32)), k
    # doubling lambda doubles L and both gradients exactly; the mean gap, the share and warped do not move
    t, _, _ = _call(dev, x, lam=2 * x["lam"])
    assert torch.equal(t["out3"][0], 2 * a["out3"][0]) and torch.equal(t["out3"][1:], a["out3"][1:])
    assert torch.equal(t["g_src"], 2 * a["g_src"]) and torch.equal(t["g_ref"], 2 * a["g_ref"])
    assert torch.equal(t["warped"], a["warped"])
    # all masked (each side alone, and both): {0, 0, 0} and zero gradients
    for sides in (("acc_src",), ("acc_ref",), ("acc_src", "acc_ref")):
        y = dict(x)
        for s in sides:
            y[s] = np.full_like(x[s], 0.25)
        z, _, rc = _call(dev, y)
        assert rc == 0
        assert not z["out3"].any() and not z["g_src"].any() and not z["g_ref"].any(), sides
        assert torch.equal(z["warped"], a["warped"])


@pytest.mark.parametrize("mode", ["a4", "a8", "a12", "mix"])
@pytest.mark.parametrize("case", ["37x61_rpy", "70x130_rpy"])
def test_alignment(case, mode, gpu_device):
    x = D.inputs(case)
    a, _, _ = _call(gpu_device, x)
    m, ar, rc = _call(gpu_device, x, mode=mode)
    assert rc == 0 and ar.guards_intact() is None
    for k in a:
        assert torch.equal(a[k].view(torch.int32), m[k].view(torch.int32)), k


def test_refusal_writes_nothing(gpu_device):
    x = D.inputs("37x61_small")
    o, ar, rc = _call(gpu_device, x, short=1)
    assert rc == -1 and b"workspace too small" in G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    for k in ("out3", "warped", "g_src", "g_ref"):
        assert torch.isnan(o[k]).all(), k             # the prefill, untouched
    assert torch.isnan(ar.t["ws"]).all()


def test_one_infinite_depth_is_outside(gpu_device):
    """A +Inf source depth has a non-finite sample coordinate: that pixel is outside (warped exactly 0, nothing flows to
    it through its own coordinates), every pixel that does not tap it is computed bit for bit as without it, and the
    call stays in bounds."""
    x = dict(D.inputs("37x61_small"))
    e = D.reference("37x61_small")["truth"]
    H, W = x["H"], x["W"]
    # the pixels whose cell can hold pixel (jx, jy): sample coordinate within two pixels of it (a superset of the
    # tappers that does not depend on how a coordinate next to an integer was rounded)
    near = lambda jx, jy: ((e["Xs"] - jx).abs() < 2) & ((e["Ys"] - jy).abs() < 2) & e["inside"]  # noqa: E731
    ok = (x["acc_src"] >= 0.5) & (x["acc_ref"] >= 0.5) & (x["depth_src"] > 1) & (x["depth_ref"] > 1)
    # the first interior pixel that is unmasked, no hole, and tapped by unmasked pixels
    j = next(v * W + u for v in range(3, H - 3) for u in range(3, W - 3)
             if ok[v - 2:v + 3, u - 2:u + 3].all() and int(near(u, v).sum()) > 0)
    plain, _, _ = _call(gpu_device, x)
    ds = x["depth_src"].copy()
    ds.reshape(-1)[j] = np.inf
    x["depth_src"] = ds
    o, ar, rc = _call(gpu_device, x)
    assert rc == 0 and ar.guards_intact() is None
    tappers = near(j % W, j // W)
    exact = torch.zeros(H * W, dtype=torch.bool)
    for k in range(4):
        exact |= e["ok"][k] & (e["tap"][k] == j)
    assert 0 < int(exact.sum()) and bool((tappers | ~exact).all()) and int(tappers.sum()) <= 16
    same = (~tappers).reshape(H, W).to(gpu_device)
    same.view(-1)[j] = False
    assert float(o["warped"].view(-1)[j]) == 0.0 and float(o["g_src"].view(-1)[j]) == 0.0
    for k in ("warped", "g_ref"):
        assert torch.equal(o[k][same].view(torch.int32), plain[k][same].view(torch.int32)), k
    assert torch.isfinite(o["out3"]).all() and torch.isfinite(o["g_src"]).all() and torch.isfinite(o["g_ref"]).all()


def test_routes_are_bit_equal(gpu_device):
    """loss.delta_depth_loss (Python autograd), _capi.delta_depth_loss (ctypes) and next.delta_depth_loss (C++)."""
    dev, x = gpu_device, D.inputs("70x130_rpy")
    base, _, _ = _call(dev, x)
    t = {k: torch.from_numpy(x[k]).to(dev) for k in IMAGES}
    out3, warped, gs, gr = G._capi.delta_depth_loss(t["depth_src"], t["acc_src"], t["depth_ref"], t["acc_ref"],
                                                    x["inv_K_src"], x["K_ref"], x["T_rel"], x["lam"], want_warped=True)
    assert torch.equal(out3, base["out3"]) and torch.equal(warped, base["warped"])
    assert torch.equal(gs, base["g_src"]) and torch.equal(gr, base["g_ref"])
    ops = G.torch_ops()
    for fn, mats in ((G.delta_depth_loss, (x["inv_K_src"], x["K_ref"], x["T_rel"])),
                     (ops.next.delta_depth_loss, tuple(torch.from_numpy(np.asarray(x[k])) for k in
                                                       ("inv_K_src", "K_ref", "T_rel")))):
        d_s = t["depth_src"][None].clone().requires_grad_(True)       # [1,H,W], as the rasterizer returns it
        d_r = t["depth_ref"][None].clone().requires_grad_(True)
        loss = fn(d_s, t["acc_src"][None], d_r, t["acc_ref"][None], *mats, x["lam"])
        assert loss.dim() == 0 and torch.equal(loss, base["out3"][0])
        (3.0 * loss).backward()
        assert torch.equal(d_s.grad[0], 3.0 * base["g_src"]) and torch.equal(d_r.grad[0], 3.0 * base["g_ref"])
        # only one side asks for a gradient
        d_s2 = t["depth_src"][None].clone().requires_grad_(True)
        loss = fn(d_s2, t["acc_src"][None], t["depth_ref"][None], t["acc_ref"][None], *mats, x["lam"])
        loss.backward()
        assert torch.equal(d_s2.grad[0], base["g_src"])
    # the default lambda is the reference's 0.2 (config/basic_common.yaml:65)
    assert torch.equal(G.delta_depth_loss(t["depth_src"], t["acc_src"], t["depth_ref"], t["acc_ref"], x["inv_K_src"],
                                          x["K_ref"], x["T_rel"]), base["out3"][0])
    with pytest.raises(G.GsrError, match="bad image shape"):
        G._capi.delta_depth_loss(*(torch.ones(1, 5, device=dev),) * 4, x["inv_K_src"], x["K_ref"], x["T_rel"], 0.2)


class _Model:
    """The getters render() asks for, over leaves of a small synthetic map."""

    def __init__(self, g, dev):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)  # noqa: E731
        self.xyz = t("means3D").requires_grad_(True)
        self.opacity, self.scales, self.rot, self.shs = t("opacities"), t("scales"), t("rotations"), t("shs")

    def Get_xyz(self): return self.xyz
    def Get_opacity(self): return self.opacity
    def Get_scaling(self): return self.scales
    def Get_rotation(self): return self.rot
    def Get_features(self): return self.shs
    def Get_max_sh_degree(self): return 0


def _loop(dev, depth_gradient):
    W, H = 70, 50
    g = S.make_gaussians(300, 21, sh_degree=0, aspect=W / H, zmin=2.0, zmax=8.0)
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)          # a surface dense enough to have depth everywhere near
    model = _Model(g, dev)
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    a = math.radians(1.5)
    R2 = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
    cams = (G.Camera(np.eye(3, dtype=np.float32), (0.0, 0.0, 0.0), fovx, fovy, W, H, device=dev),
            G.Camera(R2, (0.05, 0.0, 0.02), fovx, fovy, W, H, device=dev))
    bg = torch.zeros(3, device=dev)
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        views = [G.render(c, model, bg, depth_gradient=depth_gradient) for c in cams]
    finally:
        G.set_near_far_thread(prev_nf)
    (_, d_s, a_s), (_, d_r, a_r) = views
    d_s.retain_grad()
    d_r.retain_grad()
    fx, fy = W / (2.0 * math.tan(fovx / 2.0)), H / (2.0 * math.tan(fovy / 2.0))
    K = np.array([[fx, 0, (W - 1) / 2.0], [0, fy, (H - 1) / 2.0], [0, 0, 1]], np.float64)   # the rasterizer's pixel centres
    T = G.delta_pose(cams[0].Get_R(), cams[0].Get_T(), cams[1].Get_R(), cams[1].Get_T())
    iK = np.linalg.inv(K).astype(np.float32)
    loss = G.delta_depth_loss(d_s, a_s, d_r, a_r, iK, K.astype(np.float32), T, 0.2)
    loss.backward()
    x = dict(depth_src=d_s.detach()[0].cpu().numpy(), acc_src=a_s.detach()[0].cpu().numpy(),
             depth_ref=d_r.detach()[0].cpu().numpy(), acc_ref=a_r.detach()[0].cpu().numpy(), inv_K_src=iK,
             K_ref=K.astype(np.float32), T_rel=T.numpy(), lam=0.2, H=H, W=W)
    return model, loss, d_s, d_r, x


def test_loop_feeds_the_rasterizer_backward(gpu_device):
    G.set_binning_capacity_hint(0)
    model, loss, d_s, d_r, x = _loop(gpu_device, True)
    ref = D.evaluate(x)
    got = dict(warped=ref["truth"]["warped"], grad_src=d_s.grad[0].cpu().to(F64), grad_ref=d_r.grad[0].cpu().to(F64),
               loss=float(loss.detach()), mean_gap=float(ref["truth"]["mean_gap"]), share=float(ref["truth"]["share"]))
    r = D.ratios(got, ref)
    print("loop: fragile share %.4f" % ref["fragile_share"], "unmasked %.3f" % float(ref["truth"]["share"]),
          "worst |d| / bar:", {k: round(v, 3) for k, v in r.items()})
    assert ref["fragile_share"] <= 0.01
    assert 0.2 < float(ref["truth"]["share"]) and float(loss.detach()) > 0
    assert max(r.values()) <= 1.0, r
    assert d_s.grad.any() and d_r.grad.any()
    gx = model.xyz.grad
    assert gx is not None and torch.isfinite(gx).all() and gx.any()
    # without the opt-in the term moves no Gaussian, which is the reference's behaviour
    model0, loss0, _, _, _ = _loop(gpu_device, False)
    assert torch.equal(loss0, loss)
    assert model0.xyz.grad is not None and not model0.xyz.grad.any()
