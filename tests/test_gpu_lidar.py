"""GPU tests of the fused LiDAR depth supervision (csrc/lidar.hip: gsr_lidar_depth_image, gsr_lidar_depth_loss; loss.py,
torch_next.cpp).

Against float64: the LiDAR depth image with its two counts, and out3 = {L, mean |e|, supervised share}, dL/ddepth and
dL/dacc of every case of tests/lidar_ref.py (shapes 1x1, 3x5, 37x61, 64x80 -- exactly 20 workgroups --, 70x130 and
512x640 once, where the finish walks 1280 partial sums; 0, 1, 255, 256, 257, 5 000 and 70 001 points; identity, yaw and
rpy poses; fx != fy, the principal point off centre), each held to max(2 e_ref, bar) with the bars counted from the
kernels' arithmetic in lidar_ref.py's docstring, fragile points and pixels removed from both sides and capped at 1 %.
The exact-arithmetic scenes compare bit for bit.  tests/test_lidar_ref.py checks on the CPU that the float32
restatement stays inside the same bars.  Every case prints its worst |error| / bar; DESIGN.md section 2, "LiDAR depth
supervision", is where they are recorded.

Exact properties: reproducibility bit for bit, NaN-prefilled outputs fully written, a permutation of the points gives
the same image, null gradients leave out3 unchanged, doubling lambda doubles L and both gradients exactly, an
unsupervised frame gives {0, 0, 0} and zero gradients, n == 0, every tensor and the workspace at 0/4/8/12 bytes inside
guarded allocations (tests/arena.py), a refusal writes nothing, and the ctypes, Python autograd and C++ routes agree bit
for bit.  The loop test renders a view, supervises it with the LiDAR image of a plane and follows the gradient into the
rasterizer's backward."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import lidar_ref as L
from arena import Arena, offsets
from gs_livm_amd import synthetic as S

pytestmark = pytest.mark.gpu
F64 = torch.float64
INF = float("inf")


def _mat(a, n):
    return (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:n]])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _image(dev, x, mode="a0", counts=True, points=None, max_depth=None):
    """gsr_lidar_depth_image through ctypes with every device tensor inside guarded allocations; returns
    (image copy, counts copy or None, arena, return code)."""
    lib = G.lib()
    pts = x["points"] if points is None else points
    ar = Arena(dev, offsets(mode))
    ar.put("points", torch.from_numpy(np.ascontiguousarray(pts)).to(dev))
    ar.put("image", shape=(x["H"], x["W"]))
    if counts:
        ar.put("counts", shape=(2,))
    p = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t and ar.ptr(k) else None  # noqa: E731
    rc = lib.gsr_lidar_depth_image(int(pts.shape[0]), p("points"), _mat(x["T_cw"], 12), _mat(x["K"], 9), x["H"], x["W"],
                                   x["min_depth"], x["max_depth"] if max_depth is None else max_depth, p("image"),
                                   p("counts"), _stream())
    torch.cuda.synchronize()
    cnt = ar.t["counts"].view(torch.int32).clone() if counts else None
    return ar.t["image"].clone(), cnt, ar, rc


def _loss(dev, x, lam=None, mode="a0", g_depth=True, g_acc=True, short=0, **override):
    """gsr_lidar_depth_loss through ctypes, tensors and the workspace (exactly the queried size) inside guarded
    allocations; returns ({name: tensor copy}, arena, return code)."""
    lib = G.lib()
    H, W = x["H"], x["W"]
    ar = Arena(dev, offsets(mode))
    for k in ("depth", "acc", "lidar"):
        ar.put(k, torch.from_numpy(override.get(k, x[k])).to(dev))
    ar.put("out3", shape=(3,))
    for k, want in (("g_depth", g_depth), ("g_acc", g_acc)):
        if want:
            ar.put(k, shape=(H, W))
    nbytes = int(lib.gsr_lidar_depth_loss_workspace(H, W))
    assert nbytes % 4 == 0
    ar.put("ws", shape=(nbytes // 4,))
    p = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t else None  # noqa: E731
    rc = lib.gsr_lidar_depth_loss(H, W, p("depth"), p("acc"), p("lidar"), float(x["acc_min"]),
                                  float(x["lam"] if lam is None else lam), p("out3"), p("g_depth"), p("g_acc"), p("ws"),
                                  nbytes - short, _stream())
    torch.cuda.synchronize()
    return {k: ar.t[k].clone() for k in ("out3", "g_depth", "g_acc") if k in ar.t}, ar, rc


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_image_matches_float64(case, gpu_device):
    x, ref = L.inputs(case), L.reference(case)
    img, cnt, ar, rc = _image(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    assert not torch.isnan(img).any()                       # written in full over the NaN prefill
    r = L.image_ratios(img.cpu().numpy(), int(cnt[0]), int(cnt[1]), ref)
    shares = L.fragile_shares(ref, x)
    print(case, "fragile points %.4f pixels %.4f" % shares[:2], "counts", cnt.tolist(), "worst |d| / bar:",
          {k: round(v, 3) for k, v in r.items()})
    assert max(shares[:2]) <= 0.01
    assert max(r.values()) <= 1.0, r
    assert int(cnt[1]) == int((img > 0).sum())
    if x["n"] >= 255:
        assert int(cnt[0]) > int(cnt[1]) > 0


@pytest.mark.parametrize("case", L.EXACT_NAMES)
def test_exact_scenes_bit_for_bit(case, gpu_device):
    x, ref = L.inputs(case), L.reference(case)
    want = torch.from_numpy(ref["image"].astype(np.float32))
    for mode in ("a0", "mix"):
        img, cnt, ar, rc = _image(gpu_device, x, mode=mode)
        assert rc == 0 and ar.guards_intact() is None
        assert torch.equal(_bits(img.cpu()), _bits(want))
        assert cnt.tolist() == [ref["kept"], ref["hit"]]


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_loss_matches_float64(case, gpu_device):
    x, ref = L.inputs(case), L.reference(case)
    o, ar, rc = _loss(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    for k in o:
        assert not torch.isnan(o[k]).any(), k
    got = dict(loss=float(o["out3"][0]), mean=float(o["out3"][1]), share=float(o["out3"][2]),
               grad_depth=o["g_depth"].cpu().to(F64), grad_acc=o["g_acc"].cpu().to(F64))
    r = L.loss_ratios(got, ref)
    share = L.fragile_shares(ref, x)[2]
    print(case, "fragile pixels %.4f" % share, "supervised", ref["loss"]["n_sup"], "worst |d| / bar:",
          {k: round(v, 3) for k, v in r.items()})
    assert share <= 0.01
    assert max(r.values()) <= 1.0, r
    # exactly 0 wherever the pixel is not supervised, and where e == 0
    sup = torch.from_numpy((x["lidar"] > 0) & (x["acc"] >= np.float32(x["acc_min"])))
    assert not o["g_depth"].cpu()[~sup].any() and not o["g_acc"].cpu()[~sup].any()
    zero_e = sup & torch.from_numpy(x["depth"] / x["acc"] == x["lidar"])
    assert not o["g_depth"].cpu()[zero_e].any() and not o["g_acc"].cpu()[zero_e].any()
    if ref["loss"]["n_sup"] > 1:
        assert o["g_depth"].any() and o["g_acc"].any() and float(o["out3"][0]) > 0
    if x["H"] * x["W"] >= 1000:
        assert int(zero_e.sum()) >= 2


@pytest.mark.parametrize("case", ["3x5_n255", "37x61_n257", "64x80_n5000", "70x130_n70001"])
def test_image_exact_properties(case, gpu_device):
    dev, x = gpu_device, L.inputs(case)
    a, ca, ar, rc = _image(dev, x)
    assert rc == 0 and ar.guards_intact() is None
    b, cb, _, _ = _image(dev, x)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ca, cb)          # reproducible
    # any order of the points: the same image and counts, bit for bit
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(x["n"])
        c, cc, _, rc = _image(dev, x, points=x["points"][perm])
        assert rc == 0 and torch.equal(_bits(a), _bits(c)) and torch.equal(ca, cc)
    c, _, _, rc = _image(dev, x, points=x["points"][::-1].copy())
    assert rc == 0 and torch.equal(_bits(a), _bits(c))
    # without the counts
    c, _, ar, rc = _image(dev, x, counts=False)
    assert rc == 0 and ar.guards_intact() is None and torch.equal(_bits(a), _bits(c))
    # max_depth = +inf keeps what lies beyond 10 m and still drops the infinite coordinate
    c, cc, _, rc = _image(dev, x, max_depth=INF)
    _, kept, hit, e = L.image64(x["points"], x["T_cw"], x["K"], x["H"], x["W"], x["min_depth"], INF)
    b = L.bars(e, x["H"], x["W"], x["min_depth"], INF)
    assert rc == 0 and torch.isfinite(c).all() and int(cc[0]) >= int(ca[0])
    assert kept > L.reference(case)["image"]["kept"]
    assert abs(int(cc[0]) - kept) <= int((b["P1"] | b["P2"]).sum()) and abs(int(cc[1]) - hit) <= int((~b["keep"]).sum())


def test_no_points(gpu_device):
    """n == 0 with a null and with a non-null pointer: an all-zero image and counts {0, 0}"""
    x = L.inputs("3x5_n0")
    for pts in (x["points"], None):
        lib = G.lib()
        ar = Arena(gpu_device, offsets("a4"))
        ar.put("image", shape=(x["H"], x["W"]))
        ar.put("counts", shape=(2,))
        ar.put("dummy", shape=(3,))
        rc = lib.gsr_lidar_depth_image(0, None if pts is None else C.c_void_p(ar.ptr("dummy")), _mat(x["T_cw"], 12),
                                       _mat(x["K"], 9), x["H"], x["W"], 0.2, INF, C.c_void_p(ar.ptr("image")),
                                       C.c_void_p(ar.ptr("counts")), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and ar.guards_intact() is None
        assert not _bits(ar.t["image"]).any() and not _bits(ar.t["counts"]).any()
    img = G.lidar_depth_image(torch.empty(0, 3, device=gpu_device), x["T_cw"], x["K"], 4, 6)
    assert tuple(img.shape) == (4, 6) and not img.any()


@pytest.mark.parametrize("case", ["3x5_n255", "37x61_n257", "64x80_n5000", "70x130_n70001"])
def test_loss_exact_properties(case, gpu_device):
    dev, x = gpu_device, L.inputs(case)
    a, ar, rc = _loss(dev, x)
    assert rc == 0 and ar.guards_intact() is None
    b, _, _ = _loss(dev, x)
    for k in a:                                       # reproducible; written in full over the NaN prefill
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert not torch.isnan(a[k]).any(), k
    # null gradients (each alone and both): out3 bit for bit, the other gradient too
    for gd, ga in ((False, False), (True, False), (False, True)):
        n, ar2, rc = _loss(dev, x, g_depth=gd, g_acc=ga)
        assert rc == 0 and ar2.guards_intact() is None
        for k in n:
            assert torch.equal(_bits(n[k]), _bits(a[k])), (k, gd, ga)
    # doubling lambda doubles L and both gradients exactly; the mean error and the share do not move
    t, _, _ = _loss(dev, x, lam=2 * x["lam"])
    assert torch.equal(t["out3"][0], 2 * a["out3"][0]) and torch.equal(t["out3"][1:], a["out3"][1:])
    assert torch.equal(t["g_depth"], 2 * a["g_depth"]) and torch.equal(t["g_acc"], 2 * a["g_acc"])
    # nothing supervised (no silhouette; no LiDAR return; both): {0, 0, 0} and zero gradients
    low, none = np.full_like(x["acc"], 0.25), np.zeros_like(x["lidar"])
    for ov in (dict(acc=low), dict(lidar=none), dict(acc=low, lidar=none)):
        z, _, rc = _loss(dev, x, **ov)
        assert rc == 0
        assert not _bits(z["out3"]).any() and not z["g_depth"].any() and not z["g_acc"].any(), list(ov)
    # a NaN silhouette or LiDAR value is not supervised: everything else is computed as without that pixel's term
    sup = np.nonzero(((x["lidar"] > 0) & (x["acc"] >= np.float32(x["acc_min"]))).reshape(-1))[0]
    acc = x["acc"].copy()
    acc.reshape(-1)[sup[0]] = np.nan
    z, _, rc = _loss(dev, x, acc=acc)
    assert rc == 0 and torch.isfinite(z["out3"]).all() and float(z["g_depth"].view(-1)[sup[0]]) == 0.0
    assert float(z["out3"][2]) < float(a["out3"][2]) or len(sup) == 1


@pytest.mark.parametrize("mode", ["a4", "a8", "a12", "mix"])
@pytest.mark.parametrize("case", ["37x61_n257", "70x130_n5000"])
def test_alignment(case, mode, gpu_device):
    x = L.inputs(case)
    img, cnt, _, _ = _image(gpu_device, x)
    im2, cn2, ar, rc = _image(gpu_device, x, mode=mode)
    assert rc == 0 and ar.guards_intact() is None
    assert torch.equal(_bits(img), _bits(im2)) and torch.equal(cnt, cn2)
    a, _, _ = _loss(gpu_device, x)
    m, ar, rc = _loss(gpu_device, x, mode=mode)
    assert rc == 0 and ar.guards_intact() is None
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(m[k])), k


def test_refusals_write_nothing(gpu_device):
    x = L.inputs("37x61_n257")
    o, ar, rc = _loss(gpu_device, x, short=1)
    assert rc == -1 and b"workspace too small" in G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    for k in ("out3", "g_depth", "g_acc"):
        assert torch.isnan(o[k]).all(), k             # the prefill, untouched
    assert torch.isnan(ar.t["ws"]).all()
    img, cnt, ar, rc = _image(gpu_device, x, max_depth=x["min_depth"])
    assert rc == -1 and b"bad max_depth" in G.lib().gsr_last_error()
    assert ar.guards_intact() is None and torch.isnan(img).all() and torch.isnan(ar.t["counts"]).all()


def test_routes_are_bit_equal(gpu_device):
    """ctypes, _capi / loss.py (Python autograd) and next.* (C++)."""
    dev, x = gpu_device, L.inputs("70x130_n5000")
    img, cnt, _, _ = _image(dev, x)
    base, _, _ = _loss(dev, x)
    ops = G.torch_ops()
    pts = torch.from_numpy(x["points"]).to(dev)
    T4 = np.eye(4, dtype=np.float32)
    T4[:3] = x["T_cw"]
    for fn, mats in ((G.lidar_depth_image, (x["T_cw"], x["K"])), (G.lidar_depth_image, (T4, x["K"])),
                     (ops.next.lidar_depth_image, (torch.from_numpy(x["T_cw"]), torch.from_numpy(x["K"]))),
                     (ops.next.lidar_depth_image, (torch.from_numpy(T4), torch.from_numpy(x["K"]).to(F64)))):
        got, c2 = fn(pts, *mats, x["H"], x["W"], x["min_depth"], x["max_depth"], want_counts=True)
        assert torch.equal(_bits(got), _bits(img)) and torch.equal(c2, cnt) and c2.dtype == torch.int32
        got = fn(pts, *mats, x["H"], x["W"], x["min_depth"], x["max_depth"])
        assert torch.equal(_bits(got), _bits(img))
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("depth", "acc", "lidar")}
    out3, gd, ga = G._capi.lidar_depth_loss(t["depth"], t["acc"], t["lidar"], x["acc_min"], x["lam"])
    assert torch.equal(out3, base["out3"]) and torch.equal(gd, base["g_depth"]) and torch.equal(ga, base["g_acc"])
    for fn in (G.lidar_depth_loss, ops.next.lidar_depth_loss):
        d = t["depth"][None].clone().requires_grad_(True)             # [1,H,W], as the rasterizer returns it
        a = t["acc"][None].clone().requires_grad_(True)
        loss = fn(d, a, t["lidar"], x["acc_min"], x["lam"])
        assert loss.dim() == 0 and torch.equal(loss, base["out3"][0])
        (3.0 * loss).backward()
        assert torch.equal(d.grad[0], 3.0 * base["g_depth"]) and torch.equal(a.grad[0], 3.0 * base["g_acc"])
        # only one side asks for a gradient
        a2 = t["acc"].clone().requires_grad_(True)                    # [H,W] beside a [1,H,W] depth
        loss = fn(t["depth"][None], a2, t["lidar"][None], x["acc_min"], x["lam"])
        loss.backward()
        assert torch.equal(a2.grad, base["g_acc"])
    # .parts of the Python node, and the defaults: acc_min = 0.5, lambda = 1
    one, _, _ = _loss(dev, x, lam=1.0)
    assert torch.equal(G.lidar_depth_loss(t["depth"], t["acc"], t["lidar"]), one["out3"][0])
    d = t["depth"].clone().requires_grad_(True)
    loss = G.lidar_depth_loss(d, t["acc"], t["lidar"], lambda_=x["lam"])
    assert torch.equal(loss.grad_fn.parts, base["out3"])
    with pytest.raises(G.GsrError, match="bad acc_min"):
        G._capi.lidar_depth_loss(t["depth"], t["acc"], t["lidar"], 0.0, 1.0)


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
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)          # a surface dense enough to have a silhouette
    model = _Model(g, dev)
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    a = math.radians(8.0)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
    cam = G.Camera(R, (0.05, -0.03, 0.02), fovx, fovy, W, H, device=dev)
    # the sweep: a plane 4.5 m in front of the camera, tilted, sampled about twice per pixel
    rng = np.random.default_rng(4)
    n = 2 * W * H
    zc = 4.5 + 0.3 * rng.uniform(-1, 1, n)
    pc = np.stack([rng.uniform(-0.7, 0.7, n) * zc, rng.uniform(-0.5, 0.5, n) * zc, zc], 1)
    pw = (pc @ R.astype(np.float64).T + np.array([0.05, -0.03, 0.02])).astype(np.float32)
    K, T_cw = G.raster_K(W, H, fovx, fovy), G.world_to_camera(cam)
    zl = G.lidar_depth_image(torch.from_numpy(pw).to(dev), T_cw, K, H, W)
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        _, depth, acc = G.render(cam, model, torch.zeros(3, device=dev), depth_gradient=depth_gradient)
    finally:
        G.set_near_far_thread(prev_nf)
    depth.retain_grad()
    acc.retain_grad()
    loss = G.lidar_depth_loss(depth, acc, zl, 0.5, 0.7)
    loss.backward()
    return model, loss, depth, acc, zl


def test_loop_feeds_the_rasterizer_backward(gpu_device):
    G.set_binning_capacity_hint(0)
    model, loss, depth, acc, zl = _loop(gpu_device, True)
    out3, gd, ga = G._capi.lidar_depth_loss(depth.detach().contiguous(), acc.detach().contiguous(), zl, 0.5, 0.7)
    print("loop: supervised share %.3f, mean |e| %.3f m" % (float(out3[2]), float(out3[1])))
    assert float(out3[2]) > 0.1 and float(loss.detach()) > 0 and torch.equal(loss.detach(), out3[0])
    # what arrives at the rasterizer is the C ABI's gradient, bit for bit
    assert torch.equal(_bits(depth.grad), _bits(gd)) and torch.equal(_bits(acc.grad), _bits(ga))
    assert depth.grad.any() and acc.grad.any()
    gx = model.xyz.grad
    assert gx is not None and torch.isfinite(gx).all() and gx.any()
    # without the opt-in only the silhouette route carries the term
    model0, loss0, depth0, acc0, _ = _loop(gpu_device, False)
    assert torch.equal(loss0, loss) and torch.equal(_bits(acc0.grad), _bits(acc.grad))
    g0 = model0.xyz.grad
    assert g0 is not None and torch.isfinite(g0).all() and g0.any()
    assert not torch.equal(g0, gx)
