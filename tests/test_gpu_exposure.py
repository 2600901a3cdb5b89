"""GPU tests of the exposure-compensated photometric loss (csrc/exposure.hip: k_exposure_loss_forward / _backward /
_finish, k_apply_exposure) against the float64 truth of tests/exposure_ref.py.

Compared, from identical float32 inputs and with no element left out: {L, l1, ssim} at loss_ref's bars taken at
(x', gt); dL/dimg per pixel at |g| bar_G + 2^-24 |g G|; dL/dg_c and dL/db_c at the worst-case sums of bar_G
(exposure_ref.py's docstring: nothing there is fitted to what the kernels return).  Every figure is printed as a JSON
line before it is asserted; the worst ratios measured on an MI355X are in DESIGN.md section 2.

Exact assertions (no bar): the three scalars equal photometric_loss(apply_exposure(img), gt) and dL/dimg equals the
float32 product of g and that run's gradient; at the identity everything equals the plain loss; apply_exposure equals
exposure_ref.compensate, in place too; two runs are bitwise equal; an upstream factor of 4 scales all three gradients
exactly; the LibTorch route returns the same bits; guard words keep their bits and every output word is written; the
documented refusals write nothing.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S
import arena as A
import exposure_ref as X
import loss_ref as R
import metrics_ref as M

pytestmark = pytest.mark.gpu
INVALID = -1       # GSR_ERR_INVALID_ARGUMENT (include/gsraster.h)
HALF = 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(c, dev, want_grad=True):
    return G._capi.exposure_loss(c["img"].to(dev), c["gt"].to(dev), c["e"].to(dev), c["w"].tolist(), c["lam"],
                                 want_grad=want_grad)


def _hold(c, out3, dimg, dexp, what, **info):
    res = X.ratios(c, out3, dimg, dexp)
    print(json.dumps(dict(what=what, lam=c["lam"], **info, worst_over_bar={k: float("%.4g" % v) for k, v in res.items()})))
    over = {k: v for k, v in res.items() if not v <= 1.0}
    assert not over, "%s over the bar: %s" % (what, over)     # (every quantity that is, not the first)
    return res


@pytest.mark.parametrize("name,shape,lam,ekey", X.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_every_shape_generator_and_exposure_against_float64(name, shape, lam, ekey, gpu_device):
    dev = gpu_device
    c = X.case(name, shape, lam, ekey)
    out3, dimg, dexp = _run(c, dev)
    _hold(c, out3, dimg, dexp, "exposure loss", gen=name, shape=list(shape), e=ekey)
    # the same numbers from run to run, and the three scalars without the gradient launch
    again = _run(c, dev)
    only3, none_i, none_e = _run(c, dev, want_grad=False)
    assert none_i is None and none_e is None and torch.equal(_bits(out3), _bits(only3))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((out3, dimg, dexp), again))
    # route equality, bit for bit: the compensated image through the plain loss
    img, gt, e = c["img"].to(dev), c["gt"].to(dev), c["e"].to(dev)
    xp = G.apply_exposure(img, e)
    assert torch.equal(_bits(xp.cpu()), _bits(c["xp"]))                          # = exposure_ref.compensate
    plain3, plain_g = G._capi.photometric_loss(xp, gt, c["w"].tolist(), lam)
    assert torch.equal(_bits(out3), _bits(plain3))
    assert torch.equal(_bits(dimg), _bits(e[:, 0, None, None] * plain_g))         # float32 product of g and G


@pytest.mark.parametrize("name,shape,lam", [("noise", (3, 33, 55), 0.2), ("edges", (1, 65, 109), 1.0),
                                            ("bright", (3, 7, 5), 0.0), ("dark", (1, 1, 1), 0.2)])
def test_identity_is_the_plain_loss_bit_for_bit(name, shape, lam, gpu_device):
    dev = gpu_device
    img, gt = R.make(name, shape)
    assert not bool(torch.signbit(img).any())      # (fma(1, -0, 0) is +0: the one input the identity changes)
    w = R.reference_window_1d().tolist()
    e = G.identity_exposure(shape[0], dev)
    assert e.shape == (shape[0], 2) and e.dtype == torch.float32 and torch.equal(e.cpu(), X.exposure("identity", 3)[:shape[0]])
    out3, dimg, dexp = G._capi.exposure_loss(img.to(dev), gt.to(dev), e, w, lam)
    plain3, plain_g = G._capi.photometric_loss(img.to(dev), gt.to(dev), w, lam)
    assert torch.equal(_bits(out3), _bits(plain3)) and torch.equal(_bits(dimg), _bits(plain_g))
    assert torch.equal(_bits(G.apply_exposure(img.to(dev), e)), _bits(img.to(dev)))
    t = X.truth(img, gt, e.cpu(), R.reference_window_1d(), lam)
    _hold(dict(t, lam=lam), out3, dimg, dexp, "identity", gen=name, shape=list(shape))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 7), (3, 3, 3), (3, 7, 5), (2, 33, 55), (3, 64, 64)])
@pytest.mark.parametrize("offs", [(0, 0), (4, 4), (12, 12), (8, 0), (0, 4)], ids=lambda v: "-".join(map(str, v)))
def test_apply_exposure_equals_compensate_at_every_alignment(shape, offs, gpu_device):
    """img and out at byte offsets `offs` inside guarded allocations: equal phases take the 16-byte path with scalar
    ends (per channel: an odd plane moves every channel's phase), unequal ones the scalar path; then in place."""
    dev = gpu_device
    img, _ = R.make("noise", shape)
    e = torch.tensor(X.EXPOSURES["negative"][:shape[0]], dtype=torch.float32)
    want = X.compensate(img, e)
    L = G._capi.lib()
    ar = A.Arena(dev, lambda name, i: offs[i])
    src, dst = ar.put("img", img), ar.put("out", shape=shape)
    ed = e.to(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.gsr_apply_exposure(*shape, ar.ptr("img"), ed.data_ptr(), ar.ptr("out"), stream) == 0, L.gsr_last_error()
    torch.cuda.synchronize()
    assert ar.guards_intact() is None
    assert torch.equal(_bits(dst.cpu()), _bits(want)) and torch.equal(_bits(src.cpu()), _bits(img))
    assert L.gsr_apply_exposure(*shape, ar.ptr("img"), ed.data_ptr(), ar.ptr("img"), stream) == 0   # out == img
    torch.cuda.synchronize()
    assert ar.guards_intact() is None and torch.equal(_bits(src.cpu()), _bits(want))
    # the Python surface: a new tensor, out=, in place, the shared [2] form
    x = img.to(dev)
    assert torch.equal(_bits(G.apply_exposure(x, ed).cpu()), _bits(want)) and torch.equal(x.cpu(), img)
    assert G.apply_exposure(x, ed, out=x) is x and torch.equal(_bits(x.cpu()), _bits(want))
    shared = G.apply_exposure(img.to(dev), ed[0])
    assert torch.equal(_bits(shared.cpu()), _bits(X.compensate(img, e[:1].expand(shape[0], 2).contiguous())))


def test_upstream_factor_scales_all_three_gradients_exactly(gpu_device):
    dev = gpu_device
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    gt = c["gt"].to(dev)
    leaves = lambda: (c["img"].to(dev).requires_grad_(True), c["e"].to(dev).requires_grad_(True))  # noqa: E731
    (a, ea), (b, eb) = leaves(), leaves()
    la = G.exposure_photometric_loss(a, gt, ea, 0.2)
    ga, gea = torch.autograd.grad(la, (a, ea))
    gb, geb = torch.autograd.grad(4.0 * G.exposure_photometric_loss(b, gt, eb, 0.2), (b, eb))
    assert torch.equal(_bits(4.0 * ga), _bits(gb)) and torch.equal(_bits(4.0 * gea), _bits(geb))
    out3, dimg, dexp = _run(c, dev)
    assert torch.equal(_bits(ga), _bits(dimg)) and torch.equal(_bits(gea), _bits(dexp)) and float(la.detach()) == float(out3[0])
    assert torch.equal(_bits(la.grad_fn.parts), _bits(out3))          # .parts, as on PhotometricLoss
    # only one of the two leaves: the other gradient is not returned, the first is the same
    (only_e,) = torch.autograd.grad(G.exposure_photometric_loss(c["img"].to(dev), gt, eb, 0.2), eb)
    (only_i,) = torch.autograd.grad(G.exposure_photometric_loss(b, gt, c["e"].to(dev), 0.2), b)
    assert torch.equal(_bits(only_e), _bits(dexp)) and torch.equal(_bits(only_i), _bits(dimg))
    with torch.no_grad():
        assert float(G.exposure_photometric_loss(c["img"].to(dev), gt, c["e"].to(dev), 0.2)) == float(out3[0])


def test_shared_exposure_sums_the_channels(gpu_device):
    dev = gpu_device
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    e2 = c["e"][0].clone().to(dev).requires_grad_(True)                       # [2]: (0.8, -0.05) for every channel
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    (g2,) = torch.autograd.grad(G.exposure_photometric_loss(img, gt, e2, 0.2), e2)
    each = e2.detach().expand(3, 2).contiguous()
    out3, dimg, dexp = G._capi.exposure_loss(img, gt, each, c["w"].tolist(), 0.2)
    want = dexp.double().sum(0).cpu()
    assert g2.shape == (2,)
    # two float32 additions of three numbers: a rounding each on the running sum
    assert bool(((g2.double().cpu() - want).abs() <= 2 * HALF * dexp.double().abs().sum(0).cpu()).all())
    t = X.truth(c["img"], c["gt"], each.cpu(), c["w"], 0.2)
    _hold(dict(t, lam=0.2), out3, dimg, dexp, "shared [2] exposure")


def test_log_gain(gpu_device):
    """log_gain=True at a = log g.  The gain the device uses is exp(a) as Torch computes it there: it is read back,
    held to exp's one ulp against float64, and the truth is taken at exactly that gain, so the bars of the loss and of
    dL/dimg are unchanged; dL/da = g dL/dg (autograd's one more float32 multiply) is held at |g| bar + 2^-24 |value|."""
    dev = gpu_device
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    a = torch.stack((torch.log(c["e"][:, 0]), c["e"][:, 1]), dim=1).to(dev).requires_grad_(True)
    g_dev = torch.exp(a.detach()[:, 0]).cpu()
    assert bool(((g_dev.double() - torch.exp(a.detach()[:, 0].cpu().double())).abs() <= 2.0 ** -23 * g_dev.double()).all())
    e_used = torch.stack((g_dev, c["e"][:, 1]), dim=1)
    assert X.ties(c["img"], e_used) == 0
    img = c["img"].to(dev).requires_grad_(True)
    loss = G.exposure_photometric_loss(img, c["gt"].to(dev), a, 0.2, log_gain=True)
    gi, gl = torch.autograd.grad(loss, (img, a))
    t = dict(X.truth(c["img"], c["gt"], e_used, c["w"], 0.2), lam=0.2)
    _hold(t, loss.grad_fn.parts, gi, None, "log gain")
    g64 = g_dev.double()
    want = torch.stack((g64 * t["dexp"][:, 0], t["dexp"][:, 1]), dim=1)
    bar = torch.stack((g64 * t["bar_dexp"][:, 0] + HALF * want[:, 0].abs(), t["bar_dexp"][:, 1]), dim=1)
    ratio = ((gl.double().cpu() - want).abs() / bar).max()
    print(json.dumps(dict(what="log gain, dL/d(a, b)", worst_over_bar=float("%.4g" % ratio))))
    assert float(ratio) <= 1.0


def test_non_contiguous_image(gpu_device):
    """An HWC tensor permuted to CHW: the same loss, and the gradient lands on the elements it belongs to."""
    dev = gpu_device
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    hwc = c["img"].permute(1, 2, 0).contiguous().to(dev).requires_grad_(True)
    chw = hwc.permute(2, 0, 1)
    assert not chw.is_contiguous()
    e = c["e"].to(dev).requires_grad_(True)
    loss = G.exposure_photometric_loss(chw, c["gt"].to(dev), e, 0.2)
    g, ge = torch.autograd.grad(loss, (hwc, e))
    out3, dimg, dexp = _run(c, dev)
    assert float(loss.detach()) == float(out3[0]) and torch.equal(_bits(ge), _bits(dexp))
    assert g.shape == hwc.shape and torch.equal(_bits(g.permute(2, 0, 1)), _bits(dimg))
    assert torch.equal(_bits(G.apply_exposure(chw, e).cpu()), _bits(c["xp"]))


def test_libtorch_route_returns_the_same_bits(gpu_device):
    dev = gpu_device
    nx = G.torch_ops().next
    for key in (("edges", (3, 33, 55), 0.2, "rows"), ("noise", (1, 65, 109), 1.0, "negative")):
        c = X.case(*key)
        out3, dimg, dexp = _run(c, dev)
        img, e = c["img"].to(dev).requires_grad_(True), c["e"].to(dev).requires_grad_(True)
        loss = nx.exposure_photometric_loss(img, c["gt"].to(dev), e, c["lam"])
        gi, ge = torch.autograd.grad(loss, (img, e))
        assert float(loss.detach()) == float(out3[0]) and torch.equal(_bits(gi), _bits(dimg)) and torch.equal(_bits(ge), _bits(dexp))
        assert torch.equal(_bits(nx.apply_exposure(c["img"].to(dev), c["e"].to(dev)).cpu()), _bits(c["xp"]))
        x = c["img"].to(dev)
        assert torch.equal(_bits(nx.apply_exposure(x, c["e"].to(dev), out=x).cpu()), _bits(c["xp"]))
    # the shared [2] form and the log gain go through the same Torch ops as in Python
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    for log_gain in (False, True):
        ea, eb = (c["e"][2].clone().to(dev).requires_grad_(True) for _ in range(2))
        (ga,) = torch.autograd.grad(nx.exposure_photometric_loss(img, gt, ea, 0.2, None, log_gain), ea)
        (gb,) = torch.autograd.grad(G.exposure_photometric_loss(img, gt, eb, 0.2, log_gain=log_gain), eb)
        assert torch.equal(_bits(ga), _bits(gb))
    with pytest.raises((ValueError, RuntimeError)):
        nx.exposure_photometric_loss(img, gt, c["e"][:2].to(dev), 0.2)


# ---- buffers: through the C ABI, every buffer a view at a chosen byte offset inside a NaN-patterned allocation -------
NAMES = ("img", "gt", "e", "out3", "dimg", "dexp", "ws")


def _arena(dev, c, mode):
    L = G._capi.lib()
    Cn, H, W = c["img"].shape
    nbytes = int(L.gsr_exposure_loss_workspace(Cn, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    ar = A.Arena(dev, A.offsets(mode))
    ar.put("img", c["img"]), ar.put("gt", c["gt"]), ar.put("e", c["e"])
    ar.put("out3", shape=(3,)), ar.put("dimg", shape=c["img"].shape), ar.put("dexp", shape=(Cn, 2))
    ar.put("ws", shape=(nbytes // 4,))                           # EXACTLY the bytes asked for
    return L, ar, nbytes


def _written(t):
    return not bool((t.view(torch.int32) == A.PAT).any())


@pytest.mark.parametrize("mode", ["a0", "a4", "a8", "a12", "mix"])
@pytest.mark.parametrize("key", [("edges", (3, 33, 55), 0.2, "rows"), ("noise", (1, 65, 109), 0.2, "negative")],
                         ids=lambda v: str(v).replace(" ", ""))
def test_misaligned_guarded_buffers_and_an_exact_workspace(key, mode, gpu_device):
    """Every buffer at 0 / 4 / 8 / 12 bytes (the workspace too: its float64 pairs are aligned inside it); no guard word
    changes, every output word is written, and the results are the aligned run's bit for bit."""
    dev = gpu_device
    c = X.case(*key)
    L, ar, nbytes = _arena(dev, c, mode)
    win = (C.c_float * 11)(*c["w"].tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shape = tuple(c["img"].shape)
    ref = _run(c, dev)
    for want_grad in (True, False):
        code = L.gsr_exposure_loss(*shape, ar.ptr("img"), ar.ptr("gt"), ar.ptr("e"), win, C.c_float(c["lam"]),
                                   ar.ptr("out3"), ar.ptr("dimg") if want_grad else None,
                                   ar.ptr("dexp") if want_grad else None, ar.ptr("ws"), nbytes, stream)
        torch.cuda.synchronize()
        assert code == 0, L.gsr_last_error()
        assert ar.guards_intact() is None, "guard of %s overwritten" % ar.guards_intact()
        assert torch.equal(ar.t["img"].cpu(), c["img"]) and torch.equal(ar.t["e"].cpu(), c["e"])
        assert _written(ar.t["out3"]) and torch.equal(_bits(ar.t["out3"]), _bits(ref[0]))
        if want_grad:
            assert _written(ar.t["dimg"]) and _written(ar.t["dexp"])
            assert torch.equal(_bits(ar.t["dimg"]), _bits(ref[1])) and torch.equal(_bits(ar.t["dexp"]), _bits(ref[2]))
            ar.t["out3"].view(torch.int32).fill_(A.PAT)
    _hold(c, ar.t["out3"], ar.t["dimg"], ar.t["dexp"], "guarded", mode=mode, shape=list(shape))


def test_documented_refusals_write_nothing(gpu_device):
    """Workspace one byte short, a null exposure, one gradient pointer without the other, a non-positive shape:
    GSR_ERR_INVALID_ARGUMENT before any launch (every pointer handed in is valid and large enough all the same)."""
    dev = gpu_device
    c = X.case("edges", (3, 33, 55), 0.2, "rows")
    L, ar, nbytes = _arena(dev, c, "a0")
    win = (C.c_float * 11)(*c["w"].tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(shape=(3, 33, 55), ws_bytes=nbytes, **over):
        p = {k: ar.ptr(k) for k in NAMES}
        p.update(over)
        return L.gsr_exposure_loss(*shape, p["img"], p["gt"], p["e"], win, C.c_float(0.2), p["out3"], p["dimg"],
                                   p["dexp"], p["ws"], ws_bytes, stream)
    assert call(ws_bytes=nbytes - 1) == INVALID
    assert call(e=None) == INVALID and call(img=None) == INVALID
    assert call(dimg=None) == INVALID and call(dexp=None) == INVALID
    for bad in ((0, 33, 55), (3, 0, 55), (3, 33, 0), (-1, 33, 55)):
        assert call(shape=bad) == INVALID and int(L.gsr_exposure_loss_workspace(*bad)) == 0
    assert L.gsr_apply_exposure(3, 33, 55, ar.ptr("img"), None, ar.ptr("dimg"), stream) == INVALID
    assert L.gsr_apply_exposure(3, 0, 55, ar.ptr("img"), ar.ptr("e"), ar.ptr("dimg"), stream) == INVALID
    torch.cuda.synchronize()
    for k in ("out3", "dimg", "dexp", "ws"):
        assert bool((ar.buf[k] == A.PAT).all()), "%s written by a refused call" % k
    assert call() == 0                                           # and the same arguments, complete, are accepted
    torch.cuda.synchronize()
    assert _written(ar.t["out3"]) and _written(ar.t["dimg"]) and _written(ar.t["dexp"]) and ar.guards_intact() is None


def test_profile_counts_the_launches(gpu_device):
    """Three launches with the gradients, two without; none of the plain loss's kernels."""
    dev = gpu_device
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    counts = {}
    for want in (True, False):
        _run(c, dev, want)
        G.profile_enable(True)
        try:
            _run(c, dev, want)
            G.apply_exposure(c["img"].to(dev), c["e"].to(dev))
            torch.cuda.synchronize()
        finally:
            G.profile_enable(False)
        counts[want] = {k: v[1] for k, v in G.profile_read().items() if v[1]}
    assert counts[True] == dict(k_exposure_loss_forward=1, k_exposure_loss_backward=1, k_exposure_loss_finish=1,
                                k_apply_exposure=1)
    assert counts[False] == dict(k_exposure_loss_forward=1, k_exposure_loss_finish=1, k_apply_exposure=1)


# ---- evaluate_keyframes(exposures=...) -----------------------------------------------------------------------------
class _Model:
    """The getters render() asks for, over the tensors of a small synthetic map."""

    def __init__(self, g, dev, colour_shift=0.0):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)  # noqa: E731
        self.xyz, self.opacity, self.scales, self.rot = t("means3D"), t("opacities"), t("scales"), t("rotations")
        self.shs = t("shs")
        if colour_shift:
            gen = torch.Generator().manual_seed(17)
            self.shs = self.shs + colour_shift * (torch.rand(self.shs.shape, generator=gen) - 0.5).to(dev)

    def Get_xyz(self): return self.xyz
    def Get_opacity(self): return self.opacity
    def Get_scaling(self): return self.scales
    def Get_rotation(self): return self.rot
    def Get_features(self): return self.shs
    def Get_max_sh_degree(self): return 0


def test_evaluate_keyframes_with_exposures(gpu_device):
    """Two 48 x 64 keyframes of a synthetic scene; the camera of the second one had a gain of 1.3 (its ground truth is
    the radiance times 1.3).  Without its exposure the keyframe's PSNR is charged for the gain; with exposure
    (1.3, 0) it is restored to that of the run without the gain.  For ground truths rendered from the evaluated model
    that is +inf on both sides (metrics_ref's bar of an infinite PSNR is equality: fma(1.3, x, 0) IS the float32
    product); for a model that differs the rows are image_metrics on the compensated render, bit for bit, inside
    metrics_ref's bars at (compensate(render), ground truth)."""
    dev = gpu_device
    G.set_binning_capacity_hint(0)
    W, H = 64, 48
    g = S.make_gaussians(300, 21, sh_degree=0, aspect=W / H, zmin=2.0, zmax=8.0)
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    cams = []
    for deg in (-2.0, 3.0):
        a = math.radians(deg)
        Rm = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
        cams.append(G.Camera(Rm, (0.02 * deg, 0.0, 0.0), fovx, fovy, W, H, device=dev))
    bg = torch.full((3,), 0.1, device=dev)
    model, other = _Model(g, dev), _Model(g, dev, colour_shift=0.3)
    gain = torch.tensor([1.3, 0.0], device=dev)
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        with torch.no_grad():
            images = [G.render(c, model, bg)[0] for c in cams]
            same_gts = [images[0].clone(), images[1] * 1.3]
            other_gts = [G.render(c, other, bg)[0] for c in cams]
            other_gts[1] = other_gts[1] * 1.3
        unscaled = G.evaluate_keyframes(cams, images, model, bg)
        charged = G.evaluate_keyframes(cams, same_gts, model, bg)
        seen = []
        restored = G.evaluate_keyframes(cams, same_gts, model, bg, exposures=[None, gain],
                                        on_frame=lambda i, im, dp: seen.append(im.clone()))
        plain = G.evaluate_keyframes(cams, other_gts, model, bg)
        nones = G.evaluate_keyframes(cams, other_gts, model, bg, exposures=[None, None])
        fitted = G.evaluate_keyframes(cams, other_gts, model, bg, exposures=iter([None, gain.expand(3, 2)]))
        with pytest.raises(ValueError):
            G.evaluate_keyframes(cams, other_gts, model, bg, exposures=[gain])
    finally:
        G.set_near_far_thread(prev_nf)
    assert float(unscaled["rows"][1][0]) == math.inf and math.isfinite(float(charged["rows"][1][0]))
    assert torch.equal(_bits(restored["rows"]), _bits(unscaled["rows"])) and restored["mean_psnr"] == math.inf
    assert torch.equal(_bits(seen[0]), _bits(images[0])) and torch.equal(_bits(seen[1]), _bits(same_gts[1]))
    # without exposures: today's rows, which are image_metrics on render()'s images
    for i in range(2):
        assert torch.equal(_bits(plain["rows"][i]), _bits(G.image_metrics(images[i], other_gts[i]).cpu()))
    assert torch.equal(_bits(plain["rows"]), _bits(nones["rows"])) and torch.equal(plain["totals"], nones["totals"])
    assert torch.equal(_bits(fitted["rows"][0]), _bits(plain["rows"][0]))
    comp = G.apply_exposure(images[1], gain)
    assert torch.equal(_bits(fitted["rows"][1]), _bits(G.image_metrics(comp, other_gts[1]).cpu()))
    w = R.reference_window_1d()
    x, y = X.compensate(images[1].cpu(), torch.tensor([[1.3, 0.0]] * 3)), other_gts[1].cpu()
    assert torch.equal(_bits(comp.cpu()), _bits(x))
    r64, r32 = M.metrics(x, y, w, torch.float64), M.metrics(x, y, w, torch.float32)
    res = M.ratios(fitted["rows"][1], r64, M.bars(r64, r32, M.floors(x, y, w, r64)))
    print(json.dumps(dict(what="evaluate_keyframes, exposure", worst_over_bar={k: float("%.4g" % v[3]) for k, v in res.items()},
                          psnr_charged=float(plain["rows"][1][0]), psnr_compensated=float(fitted["rows"][1][0]))))
    assert all(v[3] <= 1.0 for v in res.values()), res
    assert float(fitted["rows"][1][0]) > float(plain["rows"][1][0])      # the gain no longer counts as error


def test_adam_fit_of_the_exposure_alone(gpu_device):
    """30 Adam steps (lr 0.005, chosen on the CPU in float64: each step lowers the loss by more than 1e-3) on e alone
    against gt = 1.3 img + 0.05: the loss falls at every step and (g, b) ends nearer to (1.3, 0.05) in every channel."""
    dev = gpu_device
    img, _ = R.make("noise", (3, 33, 55))
    img = img.to(dev)
    gt = 1.3 * img + 0.05
    e = G.identity_exposure(3, dev).requires_grad_(True)
    opt = torch.optim.Adam([e], lr=0.005)
    target = torch.tensor([1.3, 0.05], device=dev)
    losses, dist = [], []
    for _ in range(30):
        opt.zero_grad()
        loss = G.exposure_photometric_loss(img, gt, e, 0.2)
        loss.backward()
        losses.append(loss.detach())
        dist.append((e.detach() - target).norm(dim=1))
        opt.step()
    losses = torch.stack(losses).cpu()
    dist = torch.stack([dist[0], (e.detach() - target).norm(dim=1)]).cpu()
    print(json.dumps(dict(what="adam fit", first=float(losses[0]), last=float(losses[-1]), e=e.detach().cpu().tolist())))
    assert bool((losses[1:] < losses[:-1]).all())
    assert bool((dist[-1] < dist[0]).all())
