"""GPU tests of gsr_backward_depth: the blend backward with a gradient of the rendered depth.

Against float64: the ten outputs (the nine groups and dL_ddepths) of every scene and upstream mix of tests/depth_ref.py,
both binning modes, debug and product passes, at helpers.grad_close's bound with slack= (a float32 restatement in the
reference's own form stays at half of it: tests/test_depth_ref.py).  Both blend kernels (forced per process).  Exact
properties: g_d = 0 is gsr_backward bit for bit, reproducibility, full overwrite, zero rows, clean blobs, linearity.
A forced near/far split frame.  The three hosts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_ref as DR
import gs_livm_amd as G
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, grad_close, hip_forward

pytestmark = pytest.mark.gpu
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations", "dL_dconic", "dL_ddepths")


def _backward(sc, t, fwd, up, dev, debug=False, depth=True, prefill=None):
    """gsr_backward_depth (depth=True) or gsr_backward over one forward -> {name: device tensor}."""
    R, _, _, _, radii, geom, binning, img = fwd
    dc, da, dd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in up)
    g = G.rasterize_backward(t["bg"], t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"],
                             sc.get("scale_modifier", 1.0), t["cov3D_precomp"], t["viewmatrix"], t["projmatrix"],
                             sc["tanfovx"], sc["tanfovy"], dc, da, t["shs"], sc["sh_degree"], t["campos"], geom, R,
                             binning, img, debug, return_conic=True, grad_depth=dd if depth else None)
    return dict(zip(NAMES, g))


def _np(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _check_f64(got, r):
    for k in GRAD_NAMES + ("dL_ddepths",):
        ref = r[k].reshape(got[k].shape)
        if ref.size:
            grad_close(got[k], ref, k, slack=r["slack"][k])
    return DR.ratios(got, r, GRAD_NAMES + ("dL_ddepths",))


@pytest.mark.parametrize("mix", DR.MIXES)
@pytest.mark.parametrize("name", DR.SCENES)
def test_depth_backward_matches_f64(name, mix, gpu_device):
    sc, fr, up, r = DR.reference(name, mix)
    worst = {}
    for ref_rects in (True, False):
        for debug in (True, False):
            t, fwd = hip_forward(sc, gpu_device, debug=debug, ref_rects=ref_rects)
            got = _np(_backward(sc, t, fwd, up, gpu_device, debug=debug))
            for k, v in _check_f64(got, r).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(name, mix, "worst |d| / bar:", {k: round(v, 3) for k, v in worst.items()})
    if mix != "no_depth" and (fr.radii > 0).any():
        assert np.abs(r["dL_ddepths"]).max() > 0 and np.abs(got["dL_ddepths"]).max() > 0


def _exact_properties(sc, up, dev):
    """The exact properties of one frame (module docstring); returns the depth backward's outputs."""
    t, fwd = hip_forward(sc, dev, debug=False)
    zero = (up[0], up[1], np.zeros_like(up[2]))
    plain = _backward(sc, t, fwd, up, dev, depth=False)                 # gsr_backward alone
    g0 = _backward(sc, t, fwd, zero, dev)                               # depth entry, g_d = 0
    for k in NAMES[:-1]:
        assert torch.equal(g0[k], plain[k]), k
    assert not g0["dL_ddepths"].any()
    a = _backward(sc, t, fwd, up, dev)
    b = _backward(sc, t, fwd, up, dev)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k                               # reproducible; and the blobs were left clean
        assert not torch.isnan(a[k]).any(), k
    again = _backward(sc, t, fwd, up, dev, depth=False)                 # gsr_backward after gsr_backward_depth
    for k in NAMES[:-1]:
        assert torch.equal(again[k], plain[k]), k
    c = _backward(sc, t, fwd, up, dev)                                  # ... and the other way round
    for k in NAMES:
        assert torch.equal(c[k], a[k]), k
    hidden = fwd[4] <= 0
    for k in NAMES:
        assert not a[k][hidden].any(), k                                # rows with radii <= 0 are exactly zero
    # doubling g_d in the depth-only mix doubles every output exactly
    only = (np.zeros_like(up[0]), np.zeros_like(up[1]), up[2])
    twice = (only[0], only[1], 2.0 * up[2])
    d1, d2 = _backward(sc, t, fwd, only, dev), _backward(sc, t, fwd, twice, dev)
    for k in NAMES:
        assert torch.equal(d2[k], 2.0 * d1[k]), k
    assert d1["dL_ddepths"].any() and d1["dL_dmeans3D"].any()
    return _np(a), fwd


def test_outputs_are_fully_written(gpu_device):
    """Outputs pre-filled with NaN come back fully written (the C ABI directly: the Python host allocates its own)."""
    import ctypes as C
    sc, fr, up, _ = DR.reference("P300_70x50", "all")
    dev = gpu_device
    t, fwd = hip_forward(sc, dev, debug=False)
    R, _, _, _, radii, geom, binning, img = fwd
    P, M = sc["means3D"].shape[0], sc["shs"].shape[1]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    outs = [nan(P, 3), nan(P, 4), nan(P), nan(P, 3), nan(P, 3), nan(P, 6), nan(P, M, 3), nan(P, 3), nan(P, 4), nan(P)]
    dc, da, dd = (torch.from_numpy(a).to(dev) for a in up)
    p = lambda x: C.c_void_p(x.data_ptr()) if x.numel() else None  # noqa: E731
    rc = G.lib().gsr_backward_depth(
        P, sc["sh_degree"], M, int(getattr(R, "key", R)), p(t["bg"]), sc["W"], sc["H"], p(t["means3D"]), p(t["shs"]),
        None, p(t["scales"]), 1.0, p(t["rotations"]), None, p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]),
        sc["tanfovx"], sc["tanfovy"], p(radii), p(geom), p(binning), p(img), p(dc), p(da), p(dd),
        *[p(o) for o in outs[:9]], p(outs[9]), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert not torch.isnan(o).any(), i
    want = _backward(sc, t, fwd, up, dev)
    assert torch.equal(outs[9], want["dL_ddepths"]) and torch.equal(outs[4], want["dL_dmeans3D"])


@pytest.mark.parametrize("name", ["P7_33x17", "P300_70x50", "P2500_257x131"])
def test_exact_properties(name, gpu_device):
    sc, fr, up, r = DR.reference(name, "all")
    _exact_properties(sc, up, gpu_device)


_CHILD = r"""
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import torch
import depth_ref as DR
import test_gpu_depth_grad as T
from helpers import hip_forward
dev = torch.device("cuda:0")
for name in ("P7_33x17", "P1_64x64", "P300_70x50"):
    sc, fr, up, r = DR.reference(name, "all")
    got, _ = T._exact_properties(sc, up, dev)
    print(name, T._check_f64(got, r))
print("child ok")
"""


@pytest.mark.parametrize("knob", ["GSR_BLEND_BACKWARD_TILES", "GSR_BLEND_BACKWARD_QUADS"])
def test_both_blend_kernels(knob):
    """The first three scenes through each blend kernel, forced for a fresh process (the knobs are read once)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("GSR_BLEND_BACKWARD_TILES", None)
    env.pop("GSR_BLEND_BACKWARD_QUADS", None)
    env[knob] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(root, "tests"), root=root)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:]


def test_large_frame_takes_the_tile_kernel(gpu_device):
    """1024 x 768 = 3 072 tiles: the tile kernel by the size rule; the exact properties only."""
    sc = S.make_scene(2000, 1024, 768, 9, sh_degree=1)
    W, H = sc["W"], sc["H"]
    assert ((W + 15) // 16) * ((H + 15) // 16) == 3072
    dcol, dacc = S.make_upstream_grads(W, H, 9)
    gd = (np.random.default_rng(9).uniform(-1, 1, (1, H, W)) / 8.0).astype(np.float32)
    _exact_properties(sc, (dcol, dacc, gd), gpu_device)


def test_near_far_split_frame_is_bit_equal(gpu_device):
    """A forced split frame (tiny near budget) has a depth backward bit-equal to the one-chain frame's."""
    dev = gpu_device
    sc = S.make_scene(20_000, 320, 200, 6, sh_degree=1)
    W, H = sc["W"], sc["H"]
    dcol, dacc = S.make_upstream_grads(W, H, 6)
    gd = (np.random.default_rng(6).uniform(-1, 1, (1, H, W)) / 8.0).astype(np.float32)
    up = (dcol, dacc, gd)
    G.set_binning_capacity_hint(0)
    t0, one = hip_forward(sc, dev, debug=False)
    g1 = _backward(sc, t0, one, up, dev)
    G.set_near_far_hints(8, None)
    try:
        t1, two = hip_forward(sc, dev, debug=False, near_far=True)
        torch.cuda.synchronize()
        assert G.last_near_far()[0], "the frame was not split"
        g2 = _backward(sc, t1, two, up, dev)
    finally:
        G.set_near_far_hints(None, None)
    for k in NAMES:
        assert torch.equal(g1[k], g2[k]), k
    assert g1["dL_ddepths"].any()


def _leaves(sc, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev).requires_grad_(True)
         for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    return t


def _settings(cls, sc, dev, **kw):
    c = lambda k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev)  # noqa: E731
    return cls(image_height=sc["H"], image_width=sc["W"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], bg=c("bg"),
               scale_modifier=1.0, viewmatrix=c("viewmatrix"), projmatrix=c("projmatrix"), sh_degree=sc["sh_degree"],
               camera_center=c("campos"), prefiltered=False, **kw)


def _python_route(sc, dev, target, depth_gradient):
    from gs_livm_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    x = _leaves(sc, dev)
    rast = GaussianRasterizer(_settings(GaussianRasterizationSettings, sc, dev, depth_gradient=depth_gradient))
    color, radii, depth, acc = rast(x["means3D"], x["means2D"], x["opacities"], shs=x["shs"], scales=x["scales"],
                                    rotations=x["rotations"])
    (depth - target).abs().mean().backward()
    return x, depth.detach()


def test_hosts(gpu_device):
    """A depth L1 through the autograd hosts: Python with depth_gradient=True equals the C-ABI route; without the
    opt-in the leaves get no gradient from a depth-only loss, as before; the C++ route under set_depth_gradient(true) is
    bit-equal to the Python route."""
    dev = gpu_device
    sc, _ = DR.scene("P300_70x50")
    H, W = sc["H"], sc["W"]
    target = torch.from_numpy(np.random.default_rng(2).uniform(1.0, 4.0, (1, H, W)).astype(np.float32)).to(dev)
    G.set_binning_capacity_hint(0)
    x, depth = _python_route(sc, dev, target, True)
    # the C-ABI route with the same upstream: d mean|depth - target| / d depth
    gd = (torch.sign(depth - target) / depth.numel()).cpu().numpy()
    t, fwd = hip_forward(sc, dev, debug=False)
    assert torch.equal(fwd[2], depth)
    zero3, zero1 = np.zeros((3, H, W), np.float32), np.zeros((1, H, W), np.float32)
    want = _backward(sc, t, fwd, (zero3, zero1, gd), dev)
    assert torch.equal(x["means3D"].grad, want["dL_dmeans3D"]) and x["means3D"].grad.any()
    assert torch.equal(x["opacities"].grad, want["dL_dopacity"].reshape(-1, 1))
    assert torch.equal(x["scales"].grad, want["dL_dscales"]) and torch.equal(x["rotations"].grad, want["dL_drotations"])
    assert torch.equal(x["shs"].grad, want["dL_dsh"]) and torch.equal(x["means2D"].grad, want["dL_dmeans2D"])
    # depth_gradient=False: today's behaviour, the gradients of g_d = 0
    off, _ = _python_route(sc, dev, target, False)
    for k in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"):
        assert off[k].grad is not None and not off[k].grad.any(), k
    # the C++ host
    ops = G.torch_ops()
    y = _leaves(sc, dev)
    rast = ops.GaussianRasterizer(_settings(ops.GaussianRasterizationSettings, sc, dev))
    prev = ops.set_depth_gradient(True)
    try:
        assert prev is False
        color, radii, cdepth, acc = rast.forward(y["means3D"], y["means2D"], y["opacities"], shs=y["shs"],
                                                 scales=y["scales"], rotations=y["rotations"])
    finally:
        assert ops.set_depth_gradient(prev) is True
    (cdepth - target).abs().mean().backward()      # the switch was captured at forward time
    for k in x:
        assert torch.equal(y[k].grad, x[k].grad), k
    z = _leaves(sc, dev)
    color, radii, cdepth, acc = rast.forward(z["means3D"], z["means2D"], z["opacities"], shs=z["shs"],
                                             scales=z["scales"], rotations=z["rotations"])
    (cdepth - target).abs().mean().backward()      # switch off again: the depth gradient is ignored
    assert not z["means3D"].grad.any()
