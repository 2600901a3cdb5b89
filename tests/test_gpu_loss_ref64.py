"""GPU tests of the fused photometric loss (csrc/loss.hip: k_loss_forward, k_loss_backward, k_loss_finalize) against the
float64 restatement in tests/loss_ref.py.

Compared, from identical float32 inputs: loss, l1 and ssim separately, and dL/dimg PER PIXEL, each at
max(2 e_ref, K 2^-23 magnitude) (the three scalars: + the carried floor; a gradient pixel's e_ref: over its
neighbourhood); K, the magnitudes and the floors are derived in the docstring of loss_ref.py from the kernels' rounding
chain and are not fitted to what the kernels return.  No pixel is left out.
Every figure is printed as a JSON line before it is asserted; the worst ratios measured on an MI355X are in DESIGN.md
section 2.  Shapes: the smallest at which the 54 x 32 work unit, its 5-pixel halo, the seven-outputs-a-thread blocking
and the > 1024-partials loop of the finalize each engage (loss_ref.SEAM_SHAPES / MANY_PARTIALS); the float64 reference
runs on the CPU, so no plane exceeds 6e4 pixels.

Exact assertions (no bar): lam = 0 with img == gt gives 0.0 and an all-zero gradient; equal_but_one at lam = 0 has a
gradient that is zero off the one pixel and (1 - lam) / N on it; two runs are bitwise equal; want_grad = False returns
the same three floats; an upstream factor of 4 scales the gradient exactly; guard words around every buffer keep their
bits and every output word is written; the documented refusals write nothing.
"""
import ctypes as C
import json

import pytest
import torch

import gs_livm_amd as G
import loss_ref as R

pytestmark = pytest.mark.gpu
PAT = 0x7FC0DEAD   # a quiet NaN no kernel produces
LEAD = 4           # guard floats in front (16 bytes: keeps the base alignment)
INVALID = -1       # GSR_ERR_INVALID_ARGUMENT (include/gsraster.h)


def _run(c, dev, want_grad=True):
    out3, grad = G._capi.photometric_loss(c["img"].to(dev), c["gt"].to(dev), c["w"].tolist(), c["lam"], want_grad=want_grad)
    return out3, grad


def _hold(c, out3, grad, what, **info):
    got = dict(loss=float(out3[0]), l1=float(out3[1]), ssim=float(out3[2]), grad=grad)
    res = R.worst_ratios(got, c["r64"], c["bar"])
    print(json.dumps(dict(what=what, lam=c["lam"], **info, worst_over_bar={k: float("%.4g" % v[3]) for k, v in res.items()},
                          figures={k: ["%.3g" % x for x in v[:3]] for k, v in res.items()})))
    over = ["%s: err %.3g, e_ref %.3g, bar %.3g: %.3g of the bar" % ((k,) + v) for k, v in res.items() if not v[3] <= 1.0]
    assert not over, "%s over the bar: %s" % (what, "; ".join(over))   # (every quantity that is, not the first)
    return res


@pytest.mark.parametrize("name,shape,lam", R.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_every_generator_and_seam_against_float64(name, shape, lam, gpu_device):
    c = R.case(name, shape, lam)
    out3, grad = _run(c, gpu_device)
    _hold(c, out3, grad, "loss", gen=name, shape=list(shape))
    # the three scalars are the same numbers with and without the gradient launch, and from run to run
    again3, again = _run(c, gpu_device)
    only3, none = _run(c, gpu_device, want_grad=False)
    assert none is None and torch.equal(out3.view(torch.int32), only3.view(torch.int32))
    assert torch.equal(out3.view(torch.int32), again3.view(torch.int32)) and torch.equal(grad.view(torch.int32), again.view(torch.int32))
    if name == "equal_but_one" and lam == 0.0:
        N = grad.numel()
        want = torch.zeros(shape)
        want[R.one_pixel(shape)] = float(torch.tensor(1.0 / N, dtype=torch.float32))   # (1 - 0) * float32(1 / N) * (+1)
        assert torch.equal(grad.cpu(), want)


@pytest.mark.parametrize("shape,y,x,target,lam", R.impulse_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_impulses_against_float64(shape, y, x, target, lam, gpu_device):
    """One nonzero pixel: its SSIM gradient touches the 21 x 21 pixels around it through every tap of both passes and
    every padding decision (at the corners, the borders and either side of x = 53 | 54, y = 31 | 32)."""
    c = R.impulse_case(shape, y, x, target, lam)
    out3, grad = _run(c, gpu_device)
    _hold(c, out3, grad, "impulse", shape=list(shape), at=[y, x], target=target)
    if target == 0.0 and lam == 1.0:   # nothing outside the reach of the window: exactly zero
        far = torch.ones(shape[1:], dtype=torch.bool)
        far[max(0, y - 10):y + 11, max(0, x - 10):x + 11] = False
        assert not bool(grad.cpu()[:, far].any())


@pytest.mark.parametrize("shape", [(3, 33, 55), (1, 1, 1), (4, 38, 60)])
def test_image_equals_target_is_exactly_zero_at_lam_0(shape, gpu_device):
    _, gt = R.noise(shape)
    out3, grad = G._capi.photometric_loss(gt.to(gpu_device), gt.to(gpu_device), R.reference_window_1d().tolist(), 0.0)
    assert float(out3[0]) == 0.0 and float(out3[1]) == 0.0 and not bool(grad.any())


def test_upstream_factor_scales_the_gradient_exactly(gpu_device):
    c = R.case("edges", (3, 33, 55), 0.2)
    a = c["img"].to(gpu_device).requires_grad_(True)
    b = c["img"].to(gpu_device).requires_grad_(True)
    gt = c["gt"].to(gpu_device)
    (ga,) = torch.autograd.grad(G.photometric_loss(a, gt, 0.2), a)
    (gb,) = torch.autograd.grad(4.0 * G.photometric_loss(b, gt, 0.2), b)
    assert torch.equal((4.0 * ga).view(torch.int32), gb.view(torch.int32))
    _, raw = _run(c, gpu_device)
    assert torch.equal(ga.view(torch.int32), raw.view(torch.int32))


def test_non_contiguous_image(gpu_device):
    """An HWC tensor permuted to CHW: the same loss, and the gradient lands on the elements it belongs to."""
    c = R.case("noise", (3, 33, 55), 0.2)
    hwc = c["img"].permute(1, 2, 0).contiguous().to(gpu_device).requires_grad_(True)
    chw = hwc.permute(2, 0, 1)
    assert not chw.is_contiguous()
    loss = G.photometric_loss(chw, c["gt"].to(gpu_device), 0.2)
    (g,) = torch.autograd.grad(loss, hwc)
    out3, grad = _run(c, gpu_device)
    assert float(loss) == float(out3[0])
    assert g.shape == hwc.shape and torch.equal(g.permute(2, 0, 1).contiguous().view(torch.int32), grad.view(torch.int32))
    _hold(c, out3, g.permute(2, 0, 1), "non-contiguous")


def test_libtorch_route_returns_the_same_three_parts(gpu_device):
    nx = G.torch_ops().next
    for name, shape, lam in (("edges", (3, 33, 55), 0.2), ("bright", (1, 65, 109), 1.0), ("dark", (4, 38, 60), 0.0)):
        c = R.case(name, shape, lam)
        out3, grad = _run(c, gpu_device)
        parts = nx.photometric_loss_parts(c["img"].to(gpu_device), c["gt"].to(gpu_device), lam)
        assert parts.shape == (3,) and torch.equal(parts.view(torch.int32), out3.view(torch.int32))
        _hold(c, parts, None, "libtorch parts", gen=name, shape=list(shape))
        a = c["img"].to(gpu_device).requires_grad_(True)
        (ga,) = torch.autograd.grad(nx.photometric_loss(a, c["gt"].to(gpu_device), lam), a)
        assert torch.equal(ga.view(torch.int32), grad.view(torch.int32))


# ---- buffers: through the C ABI, every buffer a view at a chosen byte offset inside a NaN-patterned allocation -------
def _guarded(dev, nfloats, off):
    buf = torch.full((nfloats + 16,), PAT, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0 and off in (0, 4, 8, 12)
    start = LEAD + off // 4
    return buf, start, buf.view(torch.float32)[start:start + nfloats]


def _intact(buf, start, n):
    return bool((buf[:start] == PAT).all()) and bool((buf[start + n:] == PAT).all())


@pytest.mark.parametrize("offs", [(0, 0, 0, 0, 0), (4, 4, 4, 4, 4), (8, 8, 8, 8, 8), (12, 12, 12, 12, 12), (0, 4, 8, 12, 4),
                                  (12, 8, 4, 0, 8), (0, 0, 0, 0, 12)], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("name,shape", [("edges", (3, 33, 55)), ("noise", (1, 65, 109))])
def test_misaligned_guarded_buffers_and_an_exact_workspace(name, shape, offs, gpu_device):
    """img, gt, dL_dimg, out3 and the workspace at byte offsets `offs` inside larger allocations filled with a NaN
    pattern; the workspace has EXACTLY gsr_photometric_loss_workspace bytes (rounded up to whole floats: it is a multiple
    of 256).  Afterwards: every guard word keeps its bits, every word of dL_dimg and out3 has been written, and the
    results sit inside the same bars (bitwise equal to the aligned run: the arithmetic does not depend on the address)."""
    L = G._capi.lib()
    c = R.case(name, shape, 0.2)
    Cn, H, W = shape
    n = Cn * H * W
    nbytes = int(L.gsr_photometric_loss_workspace(Cn, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    bufs = {}
    for key, count, off in zip(("img", "gt", "grad", "out3", "ws"), (n, n, n, 3, nbytes // 4), offs):
        bufs[key] = _guarded(gpu_device, count, off)
    bufs["img"][2].copy_(c["img"].reshape(-1))
    bufs["gt"][2].copy_(c["gt"].reshape(-1))
    win = (C.c_float * 11)(*c["w"].tolist())
    ptr = lambda k: C.c_void_p(bufs[k][2].data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want_grad in (True, False):
        code = L.gsr_photometric_loss(Cn, H, W, ptr("img"), ptr("gt"), win, C.c_float(c["lam"]), ptr("out3"),
                                      ptr("grad") if want_grad else None, ptr("ws"), nbytes, stream)
        torch.cuda.synchronize()
        assert code == 0, L.gsr_last_error()
        for key, count in (("img", n), ("gt", n), ("grad", n), ("out3", 3), ("ws", nbytes // 4)):
            assert _intact(bufs[key][0], bufs[key][1], count), "guard of %s overwritten" % key
        assert torch.equal(bufs["img"][2].cpu(), c["img"].reshape(-1)) and torch.equal(bufs["gt"][2].cpu(), c["gt"].reshape(-1))
        out3 = bufs["out3"][2].clone()
        assert not bool((out3.view(torch.int32) == PAT).any())
        if want_grad:
            grad = bufs["grad"][2].clone().view(shape)
            assert not bool((grad.view(torch.int32) == PAT).any()), "a word of dL_dimg was not written"
            first3 = out3
        else:
            assert torch.equal(out3.view(torch.int32), first3.view(torch.int32))
    _hold(c, first3, grad, "guarded", gen=name, shape=list(shape), offs=list(offs))
    ref3, refg = _run(c, gpu_device)
    assert torch.equal(first3.view(torch.int32), ref3.view(torch.int32)) and torch.equal(grad.view(torch.int32), refg.view(torch.int32))


def test_documented_refusals_write_nothing(gpu_device):
    """Workspace one byte short, null img, non-positive shape: GSR_ERR_INVALID_ARGUMENT before any launch (every pointer
    handed in is valid and large enough all the same)."""
    L = G._capi.lib()
    Cn, H, W = 3, 33, 55
    n = Cn * H * W
    nbytes = int(L.gsr_photometric_loss_workspace(Cn, H, W))
    bufs = {k: _guarded(gpu_device, cnt, 0) for k, cnt in (("img", n), ("gt", n), ("grad", n), ("out3", 3), ("ws", nbytes // 4))}
    bufs["img"][2].fill_(0.5)
    bufs["gt"][2].fill_(0.25)
    win = (C.c_float * 11)(*R.reference_window_1d().tolist())
    p = {k: C.c_void_p(v[2].data_ptr()) for k, v in bufs.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda c, h, w, img, ws_bytes: L.gsr_photometric_loss(  # noqa: E731
        c, h, w, img, p["gt"], win, C.c_float(0.2), p["out3"], p["grad"], p["ws"], ws_bytes, stream)
    assert call(Cn, H, W, p["img"], nbytes - 1) == INVALID
    assert call(Cn, H, W, None, nbytes) == INVALID
    for bad in ((0, H, W), (Cn, 0, W), (Cn, H, 0), (-1, H, W), (Cn, H, -5)):
        assert call(*bad, p["img"], nbytes) == INVALID
        assert int(L.gsr_photometric_loss_workspace(*bad)) == 0
    torch.cuda.synchronize()
    for k in ("grad", "out3", "ws"):
        assert bool((bufs[k][0] == PAT).all()), "%s written by a refused call" % k
    assert call(Cn, H, W, p["img"], nbytes) == 0   # and the same arguments, complete, are accepted
    torch.cuda.synchronize()
    assert not bool((bufs["out3"][2].view(torch.int32) == PAT).any())
