"""GPU tests of the robust LiDAR depth supervision (csrc/lidar.hip: gsr_lidar_occlusion_filter,
gsr_lidar_depth_loss_robust; loss.py, metrics.py, torch_next.cpp).

The filter against tests/lidar_robust_ref.filter32 bit for bit, counts included: 1x1, 3x5 (smaller than the window:
clamping on all four sides), 37x61, 70x130 and 512x640 once (tile seams on both axes), radius 0..3, tol 0 and 0.05, on
structured images (a dense far plane, a sparse near surface whose edge crosses the seams, 0 / negative / NaN / +inf
entries, lone occluders that reach a tile through its halo only), one image from gsr_lidar_depth_image; NaN-prefilled
outputs fully written, radius 0 a cleaning copy, 0/4/8/12-byte placements inside guarded allocations, a refusal writes
nothing.  Filtering twice with tol = 0 may differ from filtering once (the second pass sees fewer occluders), so
idempotence is NOT asserted.  The filter and sweep admission's OCCLUDED code agree pixel for point.

The loss against float64 on every case shape of tests/lidar_ref.py at the parameters of tests/lidar_robust_ref.py, each
quantity held to max(2 e_ref, bar); every case prints its worst |error| / bar (DESIGN.md section 2 records them).  At
the identity parameters out4[0..2] and both gradients are gsr_lidar_depth_loss's bits on every case, through ctypes,
through Python with default arguments and through C++.  Exact properties: the exact cases bit for bit, two runs the
same bits, null gradients leave out4 alone, doubling lambda doubles L and both gradients exactly, clip_abs = 0 with
every e != 0 gives {0, 0, 0, candidate share}, the workspace has exactly the queried size inside guards, the three
routes agree bit for bit.  The loop test supervises a render with a filtered two-surface sweep; evaluate_keyframes
reports the depth error per keyframe in one copy."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import lidar_ref as L
import lidar_robust_ref as R
from arena import Arena, offsets
from gs_livm_amd import synthetic as S
from gs_livm_amd.seed import OCCLUDED

pytestmark = pytest.mark.gpu
F64 = torch.float64
INF = float("inf")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(torch.int32)


def _filter(dev, img, radius, tol, mode="a0", counts=True):
    """gsr_lidar_occlusion_filter through ctypes, every device tensor inside guarded allocations; returns
    (filtered copy on the host, counts list or None, arena, return code)."""
    lib = G.lib()
    H, W = img.shape
    ar = Arena(dev, offsets(mode))
    ar.put("src", torch.from_numpy(np.ascontiguousarray(img)).to(dev))
    ar.put("dst", shape=(H, W))
    if counts:
        ar.put("counts", shape=(2,))
    rc = lib.gsr_lidar_occlusion_filter(H, W, C.c_void_p(ar.ptr("src")), int(radius), float(tol),
                                        C.c_void_p(ar.ptr("dst")), C.c_void_p(ar.ptr("counts")) if counts else None,
                                        _stream())
    torch.cuda.synchronize()
    cnt = ar.t["counts"].view(torch.int32).tolist() if counts else None
    return ar.t["dst"].cpu(), cnt, ar, rc


def _check_filter(dev, img, radius, tol, mode="a0"):
    want, kept, removed = R.filter32(img, radius, tol)
    got, cnt, ar, rc = _filter(dev, img, radius, tol, mode=mode)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    assert torch.equal(_bits(ar.t["src"].cpu()), _np_bits(img))                  # the input is left alone
    bad = (_bits(got) != _np_bits(want))
    assert not bad.any(), (img.shape, radius, tol, mode, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    assert cnt == [kept, removed], (img.shape, radius, tol, cnt, kept, removed)
    return got, kept, removed


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (37, 61), (70, 130)])
def test_filter_matches_restatement(shape, gpu_device):
    img = R.filter_image(*shape)
    removed_any = 0
    for radius in (0, 1, 2, 3):
        for tol in (0.0, 0.05):
            got, kept, removed = _check_filter(gpu_device, img, radius, tol)
            removed_any += removed
            if radius == 0:                                  # a cleaning copy: nothing removed, the bits of z > 0
                with np.errstate(invalid="ignore"):
                    assert removed == 0 and torch.equal(_bits(got), _np_bits(np.where(img > 0, img, np.float32(0))))
    if shape[0] * shape[1] > 100:
        assert removed_any > 100
    print(shape, "removed over radius 1..3 and both tolerances:", removed_any)


def test_filter_matches_restatement_512x640(gpu_device):
    got, kept, removed = _check_filter(gpu_device, R.filter_image(512, 640), 3, 0.05)
    assert kept > 1000 and removed > 1000


def test_filter_halo_only_occluders(gpu_device):
    """lone near returns one pixel outside each border of the tile at (TILE_W, TILE_H) remove their neighbours inside it"""
    img = R.filter_image(70, 130)
    got, _, _ = _check_filter(gpu_device, img, 1, 0.05)
    x0, y0 = R.TILE_W, R.TILE_H
    lone = ((y0 + 4, x0 - 1), (y0 + 9, x0 + R.TILE_W), (y0 - 1, x0 + 30), (y0 + R.TILE_H, x0 + 45))
    for (y, x), (dy, dx) in zip(lone, ((0, 1), (0, -1), (1, 0), (-1, 0))):
        assert float(got[y, x]) == 1.0 and img[y + dy, x + dx] > 6.0 and float(got[y + dy, x + dx]) == 0.0


@pytest.mark.parametrize("mode", ["a4", "a8", "a12", "mix"])
def test_filter_alignment(mode, gpu_device):
    for shape in ((37, 61), (70, 130)):
        _check_filter(gpu_device, R.filter_image(*shape), 2, 0.05, mode=mode)
    # without the counts
    img = R.filter_image(37, 61)
    got, _, ar, rc = _filter(gpu_device, img, 2, 0.05, mode=mode, counts=False)
    assert rc == 0 and ar.guards_intact() is None
    assert torch.equal(_bits(got), _np_bits(R.filter32(img, 2, 0.05)[0]))


def _two_surfaces(H, W, K, rng):
    """Camera-frame points of a far wall (dense: about two per pixel) and, over the left part of the view, a near
    surface sampled on every third pixel."""
    n = 2 * H * W
    u, v = rng.uniform(-0.5, W - 0.5, n), rng.uniform(-0.5, H - 0.5, n)
    z = rng.uniform(6.0, 7.0, n)
    far = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)
    yy, xx = np.mgrid[0:H:3, 0:int(0.6 * W):3]
    zn = rng.uniform(2.0, 2.2, xx.size)
    near = np.stack([(xx.reshape(-1) - K[0, 2]) / K[0, 0] * zn, (yy.reshape(-1) - K[1, 2]) / K[1, 1] * zn, zn], 1)
    return np.concatenate([far, near]).astype(np.float32)


def test_filter_on_a_depth_image_of_two_surfaces(gpu_device):
    H, W = 70, 130
    K = L.intrinsics(H, W).astype(np.float64)
    pts = _two_surfaces(H, W, K, np.random.default_rng(5))
    T = np.eye(4, dtype=np.float32)[:3]
    zl = G.lidar_depth_image(torch.from_numpy(pts).to(gpu_device), T, K, H, W)
    img = zl.cpu().numpy()
    got, kept, removed = _check_filter(gpu_device, img, 2, 0.05)
    print("two surfaces: %d returns kept, %d removed" % (kept, removed))
    assert removed > 500 and kept > 500
    # what is left in front of the near surface is the near surface
    out, cnt = G.lidar_occlusion_filter(zl, 2, 0.05, want_counts=True)
    assert torch.equal(_bits(out.cpu()), _bits(got)) and cnt.tolist() == [kept, removed] and cnt.dtype == torch.int32
    inner = out[6:H - 6, 6:int(0.6 * W) - 6]
    assert float(inner.max()) < 3.0 and int((inner > 0).sum()) > 100


def test_filter_refusals_write_nothing(gpu_device):
    dev = gpu_device
    img = R.filter_image(37, 61)
    for kw, msg in ((dict(radius=4), b"bad radius"), (dict(tol=-1.0), b"bad tol"), (dict(tol=INF), b"bad tol")):
        got, cnt, ar, rc = _filter(dev, img, kw.get("radius", 1), kw.get("tol", 0.05))
        assert rc == -1 and msg in G.lib().gsr_last_error()
        assert ar.guards_intact() is None and torch.isnan(got).all() and torch.isnan(ar.t["counts"]).all()
    # in place, and a partial overlap
    ar = Arena(dev, offsets("a0"))
    ar.put("buf", torch.from_numpy(np.concatenate([img.reshape(-1), img.reshape(-1)])).to(dev))
    before = ar.t["buf"].clone()
    base = ar.ptr("buf")
    for shift in (0, 4, img.size * 4 - 4):
        rc = G.lib().gsr_lidar_occlusion_filter(37, 61, C.c_void_p(base), 1, 0.05, C.c_void_p(base + shift), None,
                                                _stream())
        torch.cuda.synchronize()
        assert rc == -1 and b"overlap" in G.lib().gsr_last_error()
        assert torch.equal(_bits(ar.t["buf"]), _bits(before)) and ar.guards_intact() is None
    # back to back in one buffer is not an overlap
    rc = G.lib().gsr_lidar_occlusion_filter(37, 61, C.c_void_p(base), 1, 0.05, C.c_void_p(base + img.size * 4), None,
                                            _stream())
    torch.cuda.synchronize()
    assert rc == 0 and ar.guards_intact() is None
    assert torch.equal(_bits(ar.t["buf"][img.size:].cpu()), _np_bits(R.filter32(img, 1, 0.05)[0]).view(-1))
    with pytest.raises(G.GsrError, match="bad radius"):
        G.lidar_occlusion_filter(torch.from_numpy(img).to(dev), 5, 0.05)


def test_filter_and_sweep_admission_agree(gpu_device):
    """One point per non-empty pixel at its centre with z = the image value: admission calls OCCLUDED exactly the points
    whose pixel the filter removes (identity pose, power-of-two intrinsics: the point lands in its pixel, z is exact)."""
    dev, H, W, r, tol = gpu_device, 37, 61, 2, 0.05
    img = R.filter_image(H, W)
    want, kept, removed = R.filter32(img, r, tol)
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(img > 0)
    z = img[ys, xs].astype(np.float64)
    K = L.EXACT_K.astype(np.float64)
    with np.errstate(invalid="ignore"):                      # (a +inf return on the optical axis: 0 * inf; the point is OUT)
        pts = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)
    a = G.admit_sweep(torch.from_numpy(pts).to(dev), L.EXACT_T, L.EXACT_K, H, W, depth_tol=0.1, occlusion_tol=tol,
                      lidar_depth=torch.from_numpy(img).to(dev), occlusion_radius=r, want_reasons=True)
    reasons = a.reasons.cpu().numpy()
    got, cnt, ar, rc = _filter(dev, img, r, tol)
    assert rc == 0 and cnt == [kept, removed] and removed > 50
    gone = (got.numpy()[ys, xs] == 0)
    assert np.array_equal(reasons == OCCLUDED, gone), int(((reasons == OCCLUDED) != gone).sum())
    assert a.counts[OCCLUDED] == removed
    finite = np.isfinite(z)
    assert (reasons[finite & ~gone] == 0).all()             # and everything else is admitted


# ---- the robust loss -------------------------------------------------------------------------------------------------
def _robust(dev, x, p, lam=None, mode="a0", g_depth=True, g_acc=True, short=0, **override):
    """gsr_lidar_depth_loss_robust through ctypes, tensors and the workspace (exactly the queried size) inside guarded
    allocations; returns ({name: tensor copy}, arena, return code)."""
    lib = G.lib()
    H, W = x["H"], x["W"]
    ar = Arena(dev, offsets(mode))
    for k in ("depth", "acc", "lidar"):
        ar.put(k, torch.from_numpy(override.get(k, x[k])).to(dev))
    ar.put("out4", shape=(4,))
    for k, want in (("g_depth", g_depth), ("g_acc", g_acc)):
        if want:
            ar.put(k, shape=(H, W))
    nbytes = int(lib.gsr_lidar_depth_loss_robust_workspace(H, W))
    assert nbytes % 4 == 0
    ar.put("ws", shape=(nbytes // 4,))
    q = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t else None  # noqa: E731
    rc = lib.gsr_lidar_depth_loss_robust(H, W, q("depth"), q("acc"), q("lidar"), float(x["acc_min"]),
                                         float(x["lam"] if lam is None else lam), p["huber_abs"], p["huber_rel"],
                                         p["clip_abs"], p["clip_rel"], q("out4"), q("g_depth"), q("g_acc"), q("ws"),
                                         nbytes - short, _stream())
    torch.cuda.synchronize()
    return {k: ar.t[k].clone() for k in ("out4", "g_depth", "g_acc") if k in ar.t}, ar, rc


def _plain(dev, x, mode="a0"):
    """gsr_lidar_depth_loss on the same inputs: (out3, g_depth, g_acc)."""
    lib = G.lib()
    H, W = x["H"], x["W"]
    ar = Arena(dev, offsets(mode))
    for k in ("depth", "acc", "lidar"):
        ar.put(k, torch.from_numpy(x[k]).to(dev))
    ar.put("out3", shape=(3,))
    ar.put("g_depth", shape=(H, W))
    ar.put("g_acc", shape=(H, W))
    nbytes = int(lib.gsr_lidar_depth_loss_workspace(H, W))
    ar.put("ws", shape=(nbytes // 4,))
    q = lambda k: C.c_void_p(ar.ptr(k))  # noqa: E731
    rc = lib.gsr_lidar_depth_loss(H, W, q("depth"), q("acc"), q("lidar"), float(x["acc_min"]), float(x["lam"]),
                                  q("out3"), q("g_depth"), q("g_acc"), q("ws"), nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return ar.t["out3"].clone(), ar.t["g_depth"].clone(), ar.t["g_acc"].clone()


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_loss_matches_float64(case, gpu_device):
    x, ref = R.inputs(case), R.reference(case)
    o, ar, rc = _robust(gpu_device, x, R.PARAMS)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    for k in o:
        assert not torch.isnan(o[k]).any(), k                # written in full over the NaN prefill
    out4 = o["out4"].cpu()
    got = dict(loss=float(out4[0]), mean=float(out4[1]), share=float(out4[2]), clip_share=float(out4[3]),
               grad_depth=o["g_depth"].cpu().to(F64), grad_acc=o["g_acc"].cpu().to(F64))
    r = R.loss_ratios(got, ref)
    N = x["H"] * x["W"]
    print(case, "F3 %.4f" % (ref["fragile_pixels"] / N), "quadratic", ref["n_quad"], "linear", ref["n_lin"], "clipped",
          ref["n_clip"], "worst |d| / bar:", {k: round(v, 3) for k, v in r.items()})
    assert ref["clip_fragile"] == 0 and ref["fragile_pixels"] / N <= 0.01
    assert max(r.values()) <= 1.0, r
    # exactly 0 wherever the pixel is not supervised -- the clipped ones included -- and where e == 0
    t = ref["terms"]
    gd, ga = o["g_depth"].cpu(), o["g_acc"].cpu()
    assert not gd[~t["sup"]].any() and not ga[~t["sup"]].any()
    zero_e = t["sup"] & torch.from_numpy(x["depth"] / x["acc"] == x["lidar"])
    assert not gd[zero_e].any() and not ga[zero_e].any()
    assert float(out4[2]) * N == pytest.approx(ref["n_sup"], abs=0.01) and float(out4[3]) * N == pytest.approx(ref["n_clip"], abs=0.01)
    if ref["n_sup"] > 1:
        assert gd.any() and ga.any() and float(out4[0]) > 0


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_identity_parameters_give_the_plain_loss_bits(case, gpu_device):
    dev = gpu_device
    for x in (L.inputs(case), R.inputs(case)):
        out3, gd, ga = _plain(dev, x)
        o, ar, rc = _robust(dev, x, R.IDENTITY)
        assert rc == 0 and ar.guards_intact() is None
        assert torch.equal(_bits(o["out4"][:3]), _bits(out3)) and float(o["out4"][3]) == 0.0
        assert torch.equal(_bits(o["g_depth"]), _bits(gd)) and torch.equal(_bits(o["g_acc"]), _bits(ga))


def test_identity_through_python_and_cpp(gpu_device):
    dev, x = gpu_device, L.inputs("70x130_n5000")
    out3, gd, ga = _plain(dev, x)
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("depth", "acc", "lidar")}
    ops = G.torch_ops()
    routes = (("python defaults", lambda d, a: G.lidar_depth_loss(d, a, t["lidar"], x["acc_min"], x["lam"])),
              ("python node", lambda d, a: G.RobustLidarDepthLoss.apply(d, a, t["lidar"], x["acc_min"], x["lam"], 0.0,
                                                                        0.0, INF, 0.0)),
              ("c++", lambda d, a: ops.next.lidar_depth_loss_robust(d, a, t["lidar"], x["acc_min"], x["lam"], 0.0, 0.0,
                                                                    INF, 0.0)))
    for name, fn in routes:
        d = t["depth"][None].clone().requires_grad_(True)
        a = t["acc"][None].clone().requires_grad_(True)
        loss = fn(d, a)
        assert loss.dim() == 0 and torch.equal(_bits(loss.detach()), _bits(out3[0])), name
        loss.backward()
        assert torch.equal(_bits(d.grad[0]), _bits(gd)) and torch.equal(_bits(a.grad[0]), _bits(ga)), name
    # default arguments take the existing node, any other value the robust one
    d = t["depth"].clone().requires_grad_(True)
    assert type(G.lidar_depth_loss(d, t["acc"], t["lidar"]).grad_fn).__name__.startswith("LidarDepthLoss")
    assert type(G.lidar_depth_loss(d, t["acc"], t["lidar"], huber=0.1).grad_fn).__name__.startswith("RobustLidarDepthLoss")
    assert type(G.lidar_depth_loss(d, t["acc"], t["lidar"], clip=1.0).grad_fn).__name__.startswith("RobustLidarDepthLoss")


@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_exact_cases_bit_for_bit(shape, gpu_device):
    x = R.exact_case(*shape)
    for mode in ("a0", "mix"):
        o, ar, rc = _robust(gpu_device, x, R.EXACT, mode=mode)
        assert rc == 0 and ar.guards_intact() is None
        assert torch.equal(_bits(o["out4"].cpu()), _np_bits(x["out4"])), (o["out4"].tolist(), x["out4"].tolist())
        assert torch.equal(_bits(o["g_depth"].cpu()), _np_bits(x["grad_depth"]))
        assert torch.equal(_bits(o["g_acc"].cpu()), _np_bits(x["grad_acc"]))
    if shape[0] * shape[1] > 100:
        # the pixels at exactly a == clip are supervised (the rule is >): they carry a gradient
        at_clip = torch.from_numpy(x["sup"] & (np.abs(x["depth"] - x["lidar"]) == 1 + x["lidar"] / 4))
        assert int(at_clip.sum()) > 1 and bool((o["g_depth"].cpu()[at_clip] != 0).all())


@pytest.mark.parametrize("case", ["3x5_n255", "37x61_n257", "64x80_n5000", "70x130_n70001"])
def test_loss_exact_properties(case, gpu_device):
    dev, x, p = gpu_device, R.inputs(case), R.PARAMS
    a, ar, rc = _robust(dev, x, p)
    assert rc == 0 and ar.guards_intact() is None
    b, _, _ = _robust(dev, x, p)
    for k in a:                                              # reproducible
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    # null gradients (each alone and both): out4 bit for bit, the other gradient too
    for gd, ga in ((False, False), (True, False), (False, True)):
        n, ar2, rc = _robust(dev, x, p, g_depth=gd, g_acc=ga)
        assert rc == 0 and ar2.guards_intact() is None
        for k in n:
            assert torch.equal(_bits(n[k]), _bits(a[k])), (k, gd, ga)
    # doubling lambda doubles L and both gradients exactly; the mean error and the shares do not move
    t, _, _ = _robust(dev, x, p, lam=2 * x["lam"])
    assert torch.equal(t["out4"][0], 2 * a["out4"][0]) and torch.equal(t["out4"][1:], a["out4"][1:])
    assert torch.equal(t["g_depth"], 2 * a["g_depth"]) and torch.equal(t["g_acc"], 2 * a["g_acc"])
    # clip_abs = clip_rel = 0 with every e != 0: nothing is supervised, every candidate is clipped
    cand = (x["lidar"] > 0) & (x["acc"] >= np.float32(x["acc_min"]))
    depth = np.where(cand & (x["depth"] / x["acc"] == x["lidar"]), x["depth"] * np.float32(1.25), x["depth"])
    z, _, rc = _robust(dev, x, dict(p, clip_abs=0.0, clip_rel=0.0), depth=depth.astype(np.float32))
    assert rc == 0 and not _bits(z["out4"][:3]).any() and not z["g_depth"].any() and not z["g_acc"].any()
    assert float(z["out4"][3]) == float(np.float32(np.float64(int(cand.sum())) / cand.size)) > 0
    # alignment: every tensor and the workspace at 4, 8, 12 bytes
    for mode in ("a4", "a8", "a12", "mix"):
        m, ar3, rc = _robust(dev, x, p, mode=mode)
        assert rc == 0 and ar3.guards_intact() is None
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(m[k])), (k, mode)


def test_loss_refusals_write_nothing(gpu_device):
    x = R.inputs("37x61_n257")
    o, ar, rc = _robust(gpu_device, x, R.PARAMS, short=1)
    assert rc == -1 and b"workspace too small" in G.lib().gsr_last_error()
    assert ar.guards_intact() is None and torch.isnan(ar.t["ws"]).all()
    for k in ("out4", "g_depth", "g_acc"):
        assert torch.isnan(o[k]).all(), k
    o, ar, rc = _robust(gpu_device, x, dict(R.PARAMS, huber_abs=-1.0))
    assert rc == -1 and b"bad huber_abs" in G.lib().gsr_last_error() and torch.isnan(o["out4"]).all()


def test_routes_are_bit_equal(gpu_device):
    """ctypes, _capi / loss.py (Python autograd) and next.* (C++), at the robust parameters"""
    dev, x, p = gpu_device, R.inputs("70x130_n5000"), R.PARAMS
    base, _, _ = _robust(dev, x, p)
    ops = G.torch_ops()
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("depth", "acc", "lidar")}
    out4, gd, ga = G._capi.lidar_depth_loss_robust(t["depth"], t["acc"], t["lidar"], x["acc_min"], x["lam"],
                                                   p["huber_abs"], p["huber_rel"], p["clip_abs"], p["clip_rel"])
    assert torch.equal(_bits(out4), _bits(base["out4"])) and torch.equal(gd, base["g_depth"]) and torch.equal(ga, base["g_acc"])
    py = lambda d, a: G.lidar_depth_loss(d, a, t["lidar"], x["acc_min"], x["lam"], huber=p["huber_abs"],  # noqa: E731
                                         huber_rel=p["huber_rel"], clip=p["clip_abs"], clip_rel=p["clip_rel"])
    cpp = lambda d, a: ops.next.lidar_depth_loss_robust(d, a, t["lidar"], x["acc_min"], x["lam"], p["huber_abs"],  # noqa: E731
                                                        p["huber_rel"], p["clip_abs"], p["clip_rel"])
    for fn in (py, cpp):
        d = t["depth"][None].clone().requires_grad_(True)             # [1,H,W], as the rasterizer returns it
        a = t["acc"][None].clone().requires_grad_(True)
        loss = fn(d, a)
        assert loss.dim() == 0 and torch.equal(loss.detach(), base["out4"][0])
        (3.0 * loss).backward()                                       # one node, scaled by the upstream scalar
        assert torch.equal(d.grad[0], 3.0 * base["g_depth"]) and torch.equal(a.grad[0], 3.0 * base["g_acc"])
        a2 = t["acc"].clone().requires_grad_(True)                    # only one side asks for a gradient
        fn(t["depth"][None], a2).backward()
        assert torch.equal(a2.grad, base["g_acc"])
    d = t["depth"].clone().requires_grad_(True)
    loss = py(d, t["acc"])
    assert torch.equal(_bits(loss.grad_fn.parts), _bits(base["out4"]))
    # the filter through Python and C++
    img = torch.from_numpy(R.filter_image(70, 130)).to(dev)
    want = _np_bits(R.filter32(R.filter_image(70, 130), 3, 0.05)[0])
    for fn in (G.lidar_occlusion_filter, ops.next.lidar_occlusion_filter):
        out, cnt = fn(img, 3, 0.05, want_counts=True)
        assert torch.equal(_bits(out.cpu()), want) and cnt.dtype == torch.int32 and int(cnt.sum()) == int((img > 0).sum())
        assert torch.equal(_bits(fn(img[None], 3, 0.05).cpu())[0], want)
    with pytest.raises(G.GsrError, match="bad clip_abs"):
        G.lidar_depth_loss(t["depth"], t["acc"], t["lidar"], clip=-1.0)


# ---- the loop: render, filtered two-surface sweep, one backward ---------------------------------------------------------
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


def _scene(dev, W=70, H=50):
    g = S.make_gaussians(300, 21, sh_degree=0, aspect=W / H, zmin=2.0, zmax=8.0)
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)          # a surface dense enough to have a silhouette
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    return g, fovx, fovy


def test_loop_filtered_pixels_carry_no_gradient(gpu_device):
    dev, W, H = gpu_device, 70, 50
    G.set_binning_capacity_hint(0)
    g, fovx, fovy = _scene(dev, W, H)
    model = _Model(g, dev)
    cam = G.Camera(np.eye(3, dtype=np.float32), (0.0, 0.0, 0.0), fovx, fovy, W, H, device=dev)
    K, T_cw = G.raster_K(W, H, fovx, fovy), G.world_to_camera(cam)
    pts = _two_surfaces(H, W, K.numpy(), np.random.default_rng(6))
    zl = G.lidar_depth_image(torch.from_numpy(pts).to(dev), T_cw, K, H, W)
    zf, cnt = G.lidar_occlusion_filter(zl, 2, 0.05, want_counts=True)
    removed = (zl > 0) & (zf == 0)
    assert int(cnt[1]) == int(removed.sum()) > 100
    grads = {}
    for name, image in (("filtered", zf), ("raw", zl)):
        prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
        try:
            _, depth, acc = G.render(cam, model, torch.zeros(3, device=dev), depth_gradient=True)
        finally:
            G.set_near_far_thread(prev_nf)
        depth.retain_grad()
        loss = G.lidar_depth_loss(depth, acc, image, 0.5, 0.7, huber=0.1, clip=20.0)
        model.xyz.grad = None
        loss.backward()
        grads[name] = depth.grad.reshape(H, W).clone()
        assert torch.isfinite(model.xyz.grad).all() and model.xyz.grad.any()
    lit = removed & (acc.detach().reshape(H, W) >= 0.5)
    assert int(lit.sum()) > 20
    assert not grads["filtered"][removed].any()                    # exactly zero where the filter removed the return
    assert bool((grads["raw"][lit] != 0).all())                    # and pulled towards the far wall without the filter


# ---- evaluate_keyframes(lidar_depths=...) -----------------------------------------------------------------------------
def test_evaluate_keyframes_with_lidar_depths(gpu_device):
    dev, W, H = gpu_device, 64, 48
    G.set_binning_capacity_hint(0)
    g, fovx, fovy = _scene(dev, W, H)
    model = _Model(g, dev)
    model.xyz.requires_grad_(False)
    cams = []
    for deg in (-2.0, 0.0, 3.0):
        a = math.radians(deg)
        Rm = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
        cams.append(G.Camera(Rm, (0.02 * deg, 0.0, 0.0), fovx, fovy, W, H, device=dev))
    bg = torch.full((3,), 0.1, device=dev)
    gen = torch.Generator().manual_seed(3)
    prev_nf = G.set_near_far_thread(False)
    try:
        with torch.no_grad():
            frames = [G.render(c, model, bg) for c in cams]
        gts = [(f[0] + 0.05 * torch.rand(f[0].shape, generator=gen).to(dev)).clamp(0, 1) for f in frames]
        # a LiDAR image per keyframe: the render's own depth off by a few centimetres on two pixels in three
        zls = []
        for f in frames:
            d, a = f[1].reshape(H, W), f[2].reshape(H, W)
            zl = torch.where(a > 0.3, d / a.clamp_min(1e-6) + 0.03, torch.zeros_like(d))
            zl.view(-1)[::3] = 0.0
            zls.append(zl.contiguous())
        plain = G.evaluate_keyframes(cams, gts, model, bg)
        res = G.evaluate_keyframes(cams, gts, model, bg, lidar_depths=[zls[0], None, zls[2]])
        none = G.evaluate_keyframes(cams, gts, model, bg, lidar_depths=[None, None, None])
        with pytest.raises(ValueError):
            G.evaluate_keyframes(cams, gts, model, bg, lidar_depths=[zls[0]])
    finally:
        G.set_near_far_thread(prev_nf)
    assert set(plain) == {"rows", "totals", "mean_psnr", "mean_ssim", "frames"}
    assert set(res) == set(plain) | {"depth_rows", "mean_depth_error"}
    assert torch.equal(_bits(res["rows"]), _bits(plain["rows"])) and torch.equal(res["totals"], plain["totals"])
    assert res["mean_psnr"] == plain["mean_psnr"] and res["mean_ssim"] == plain["mean_ssim"]
    dr = res["depth_rows"]
    assert tuple(dr.shape) == (3, 4) and dr.dtype == torch.float32 and not dr.is_cuda
    assert torch.isnan(dr[1]).all()
    for i in (0, 2):
        out4, _, _ = G._capi.lidar_depth_loss_robust(frames[i][1].contiguous(), frames[i][2].contiguous(), zls[i], 0.5,
                                                     1.0, 0.0, 0.0, INF, 0.0, want_grad_depth=False, want_grad_acc=False)
        assert torch.equal(_bits(dr[i]), _bits(out4.cpu())), i
        assert 0.02 < float(dr[i][1]) < 0.04 and float(dr[i][2]) > 0.1 and float(dr[i][3]) == 0.0
    assert res["mean_depth_error"] == float(dr[[0, 2], 1].double().mean())
    assert torch.isnan(none["depth_rows"]).all() and math.isnan(none["mean_depth_error"])
