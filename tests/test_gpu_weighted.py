"""GPU tests of the weighted photometric loss (csrc/weighted.hip: k_weighted_loss_forward / _backward / _finish) against the float64 truth of tests/weighted_ref.py.

Compared, from identical float32 inputs and with no element left out: out6 = {L, l1, ssim, S, mse, psnr}, dL/dimg per
pixel and dL/dexposure at weighted_ref's bars (max(2 e_ref, floor); nothing there is fitted to what the kernels return).
Every figure is printed as a JSON line before it is asserted; the worst ratios measured on an MI355X are in DESIGN.md
section 2 and profiles/weighted_loss_ratios.txt.

Exact assertions (no bar): (a) with ones, given or absent, {L, l1, ssim} and the gradients are gsr_exposure_loss's, and
gsr_photometric_loss's without an exposure; (b) a {0, 1} map equals the same mask from the acc gate; (c) weights times
4 and 2^-3 change S and nothing else; (d) the gradient is zero where no weight lies within 5 pixels; (e) data more than
5 pixels from every weighted pixel reaches no output bit; (f) all-zero weights give the specified outputs; (g) two runs
agree and want_grad=False gives the same out6; (h) an upstream factor of 4 scales both gradients exactly; (i) the
LibTorch route returns the same bits; (j) image_metrics(weights=) is out6's entries, and today's call without; (k)
guard words keep their bits and every output word is written.  The mutants of the definition are refused on the CPU
(test_weighted_ref.py).
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gs_livm_amd as G
from gs_livm_amd import synthetic as S
import arena as A
import loss_ref as R
import weighted_ref as Q

pytestmark = pytest.mark.gpu
IDS = lambda v: str(v).replace(" ", "")  # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _dev(t, dev):
    return None if t is None else t.to(dev)


def _run(c, dev, want_grad=True, **over):
    p = dict(img=c["img"], gt=c["gt"], weights=c["weights"], acc=c["acc"], e=c["e"])
    p.update(over)
    return G._capi.weighted_loss(p["img"].to(dev), p["gt"].to(dev), _dev(p["weights"], dev), _dev(p["acc"], dev),
                                 Q.ACC_MIN, _dev(p["e"], dev), c["win"].tolist(), c["lam"], want_grad=want_grad)


def _hold(c, out6, dimg, dexp, what, **info):
    res = Q.ratios(c, out6.cpu(), dimg, dexp)
    print(json.dumps(dict(what=what, lam=c["lam"], **info, worst_over_bar={k: float("%.4g" % v) for k, v in res.items()})))
    over = {k: v for k, v in res.items() if not v <= 1.0}
    assert not over, "%s over the bar: %s" % (what, over)     # (every quantity that is, not the first)
    return res


# ---- 1. against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,lam,pat,ekey", Q.CASES, ids=IDS)
def test_every_shape_pattern_and_exposure_against_float64(name, shape, lam, pat, ekey, gpu_device):
    dev = gpu_device
    c = Q.case(name, shape, lam, pat, ekey)
    out6, dimg, dexp = _run(c, dev)
    assert (dexp is None) == (ekey is None)
    _hold(c, out6, dimg, dexp, "weighted loss", gen=name, shape=list(shape), pattern=pat, e=ekey)
    # (g) the same numbers from run to run, and out6 without the gradient launches
    only6, none_i, none_e = _run(c, dev, want_grad=False)
    assert none_i is None and none_e is None and torch.equal(_bits(out6), _bits(only6))
    assert _same((out6, dimg, dexp), _run(c, dev))
    if pat == "zero":  # (f)
        assert out6.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, math.inf]
        assert not bool(dimg.any()) and (dexp is None or not bool(dexp.any()))


# ---- 2. equalities, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen,shape,lam", [("noise", (3, 33, 55), 0.2), ("edges", (1, 65, 109), 1.0),
                                           ("bright", (3, 7, 5), 0.0), ("dark", (1, 1, 1), 0.2),
                                           ("edges", Q.MANY, 0.2)], ids=IDS)
def test_a_ones_are_the_exposure_loss_and_the_plain_loss(gen, shape, lam, gpu_device):
    dev = gpu_device
    img, gt = (t.to(dev) for t in R.make(gen, shape))
    win = R.reference_window_1d().tolist()
    ones = torch.ones(shape[1:], device=dev)
    for ekey in ("rows", "negative"):
        e = Q.exposure(ekey, shape[0]).to(dev)
        want3, want_i, want_e = G._capi.exposure_loss(img, gt, e, win, lam)
        for w in (ones, None):
            out6, dimg, dexp = G._capi.weighted_loss(img, gt, w, None, Q.ACC_MIN, e, win, lam)
            assert torch.equal(_bits(out6[:3]), _bits(want3)), (ekey, w is None)
            assert torch.equal(_bits(dimg), _bits(want_i)) and torch.equal(_bits(dexp), _bits(want_e)), (ekey, w is None)
            assert float(out6[3]) == shape[1] * shape[2]
    plain3, plain_g = G._capi.photometric_loss(img, gt, win, lam)
    for w in (ones, None):
        out6, dimg, dexp = G._capi.weighted_loss(img, gt, w, None, Q.ACC_MIN, None, win, lam)
        assert dexp is None and torch.equal(_bits(out6[:3]), _bits(plain3)) and torch.equal(_bits(dimg), _bits(plain_g))
        only6, _, _ = G._capi.weighted_loss(img, gt, w, None, Q.ACC_MIN, None, win, lam, want_grad=False)
        assert torch.equal(_bits(only6), _bits(out6))


@pytest.mark.parametrize("ekey", [None, "rows"])
def test_b_a_binary_map_is_the_same_mask_from_the_gate(ekey, gpu_device):
    dev = gpu_device
    c = Q.case("noise", (3, 33, 55), 0.2, "gate", ekey)
    mask = (c["w"] > 0).float()                                   # where the gate is open and the ramp is not 0
    gate = (c["acc"] >= Q.ACC_MIN).float()
    ref = _run(c, dev, weights=mask, acc=None)
    assert _same(ref, _run(c, dev, weights=None, acc=mask))                       # acc in {0, 1} against acc_min = 0.5
    assert _same(_run(c, dev, weights=gate, acc=None), _run(c, dev, weights=None))  # the gate alone, NaN included
    assert _same(_run(c, dev, weights=c["w"], acc=None), _run(c, dev))             # ramp times gate, both ways
    assert float(ref[0][3]) == float(mask.sum())


@pytest.mark.parametrize("pat,ekey", [("ramp", "negative"), ("frame", None), ("gate", "rows")])
def test_c_a_power_of_two_on_the_weights_scales_S_and_nothing_else(pat, ekey, gpu_device):
    dev = gpu_device
    c = Q.case("noise", (3, 33, 55), 0.2, pat, ekey)
    out6, dimg, dexp = _run(c, dev)
    for s in (4.0, 0.125):
        o, di, de = _run(c, dev, weights=c["weights"] * s)
        keep = [0, 1, 2, 4, 5]
        assert torch.equal(_bits(o[keep]), _bits(out6[keep])) and float(o[3]) == s * float(out6[3])
        assert _same((di, de), (dimg, dexp))


def _near(w, reach=5):
    """[H,W] bool: some weight within `reach` pixels (Chebyshev)"""
    return F.max_pool2d((w > 0).float()[None, None], 2 * reach + 1, stride=1, padding=reach)[0, 0] > 0


@pytest.mark.parametrize("pat,ekey", [("frame", "rows"), ("blocks", None), ("seam", "negative"), ("corner", None)])
def test_d_e_data_far_from_every_weighted_pixel_reaches_no_output(pat, ekey, gpu_device):
    dev = gpu_device
    c = Q.case("noise", (1, 65, 109), 0.2, pat, ekey)
    ref = _run(c, dev)
    far = ~_near(c["w"])
    assert bool(far.any()) and bool((~far).any())
    assert not bool(ref[1][:, far.to(dev)].any())                 # (d): exactly zero
    gen = torch.Generator().manual_seed(5)
    img, gt = c["img"].clone(), c["gt"].clone()
    img[:, far] = 3.0 * torch.rand(img[:, far].shape, generator=gen) - 1.0     # other values, other signs of x - y
    gt[:, far] = torch.rand(gt[:, far].shape, generator=gen)
    assert _same(ref, _run(c, dev, img=img, gt=gt))               # (e)
    # and the pixel just inside the reach does count
    edge = _near(c["w"]) & ~_near(c["w"], 4)
    img2 = c["img"].clone()
    img2[:, edge] += 0.25
    assert not torch.equal(_bits(_run(c, dev, img=img2)[0]), _bits(ref[0]))


def test_f_all_zero_from_the_gate_and_non_finite_free(gpu_device):
    dev = gpu_device
    c = Q.case("bright", (3, 33, 55), 0.2, "ramp", "negative")
    for kw in (dict(acc=torch.full((33, 55), 0.25)), dict(acc=torch.full((33, 55), float("nan"))),
               dict(weights=torch.zeros((33, 55)))):
        out6, dimg, dexp = _run(c, dev, **kw)
        assert out6.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, math.inf]
        assert not bool(dimg.any()) and not bool(dexp.any())


def test_h_upstream_factor_and_the_autograd_surface(gpu_device):
    dev = gpu_device
    c = Q.case("noise", (3, 33, 55), 0.2, "gate", "rows")
    gt, w, acc = c["gt"].to(dev), c["weights"].to(dev), c["acc"].to(dev)
    leaves = lambda: (c["img"].to(dev).requires_grad_(True), c["e"].to(dev).requires_grad_(True))  # noqa: E731
    (a, ea), (b, eb) = leaves(), leaves()
    la = G.weighted_photometric_loss(a, gt, w, acc, Q.ACC_MIN, ea, 0.2)
    ga, gea = torch.autograd.grad(la, (a, ea))
    gb, geb = torch.autograd.grad(4.0 * G.weighted_photometric_loss(b, gt, w, acc, Q.ACC_MIN, eb, 0.2), (b, eb))
    assert torch.equal(_bits(4.0 * ga), _bits(gb)) and torch.equal(_bits(4.0 * gea), _bits(geb))
    out6, dimg, dexp = _run(c, dev)
    assert torch.equal(_bits(ga), _bits(dimg)) and torch.equal(_bits(gea), _bits(dexp))
    assert la.grad_fn.parts.shape == (6,) and torch.equal(_bits(la.grad_fn.parts), _bits(out6))
    # acc may be the live render output ([1,H,W], part of a graph): detached, not refused; no gradient reaches it
    live = acc[None].clone().requires_grad_(True) * 1.0
    wl = w.clone().requires_grad_(True)
    (gi,) = torch.autograd.grad(G.weighted_photometric_loss(b, gt, wl, live, Q.ACC_MIN, c["e"].to(dev), 0.2), b)
    assert torch.equal(_bits(gi), _bits(dimg))
    # only the exposure; no exposure at all; the shared [2] form and the log gain
    (only_e,) = torch.autograd.grad(G.weighted_photometric_loss(c["img"].to(dev), gt, w, acc, Q.ACC_MIN, eb, 0.2), eb)
    assert torch.equal(_bits(only_e), _bits(dexp))
    plain = G.weighted_photometric_loss(b, gt, w, acc)
    (gp,) = torch.autograd.grad(plain, b)
    want = _run(c, dev, e=None)
    assert torch.equal(_bits(gp), _bits(want[1])) and torch.equal(_bits(plain.grad_fn.parts), _bits(want[0]))
    e2 = c["e"][0].clone().to(dev).requires_grad_(True)
    (g2,) = torch.autograd.grad(G.weighted_photometric_loss(b, gt, w, acc, exposure=e2), e2)
    each = _run(c, dev, e=c["e"][0].expand(3, 2).contiguous())[2]
    assert g2.shape == (2,) and bool(((g2.double() - each.double().sum(0)).abs() <= 2 * Q.HALF * each.double().abs().sum(0)).all())
    lg = torch.stack((torch.log(c["e"][:, 0]), c["e"][:, 1]), dim=1).to(dev).requires_grad_(True)
    ll = G.weighted_photometric_loss(b, gt, w, acc, exposure=lg, log_gain=True)
    assert abs(float(ll.detach()) - float(out6[0])) <= 1e-5
    with torch.no_grad():
        assert float(G.weighted_photometric_loss(c["img"].to(dev), gt, w, acc, Q.ACC_MIN, c["e"].to(dev), 0.2)) == float(out6[0])


def test_i_libtorch_route_returns_the_same_bits(gpu_device):
    dev = gpu_device
    nx = G.torch_ops().next
    for key in (("edges", (3, 33, 55), 0.2, "gate", "rows"), ("noise", (1, 65, 109), 1.0, "frame", None),
                ("noise", (3, 33, 55), 0.2, "zero", "negative")):
        c = Q.case(*key)
        out6, dimg, dexp = _run(c, dev)
        img = c["img"].to(dev).requires_grad_(True)
        e = None if c["e"] is None else c["e"].to(dev).requires_grad_(True)
        args = (c["gt"].to(dev), _dev(c["weights"], dev), _dev(c["acc"], dev), Q.ACC_MIN)
        loss = nx.weighted_photometric_loss(img, *args, e, c["lam"])
        grads = torch.autograd.grad(loss, (img,) if e is None else (img, e))
        assert float(loss.detach()) == float(out6[0]) and torch.equal(_bits(grads[0]), _bits(dimg))
        assert e is None or torch.equal(_bits(grads[1]), _bits(dexp))
        parts = nx.weighted_photometric_loss_parts(c["img"].to(dev), *args, _dev(c["e"], dev), c["lam"])
        assert torch.equal(_bits(parts), _bits(out6))
        if c["acc"] is None:
            m = nx.image_metrics(c["img"].to(dev), c["gt"].to(dev), None, None, c["weights"].to(dev))
            assert torch.equal(_bits(m), _bits(G.image_metrics(c["img"].to(dev), c["gt"].to(dev), weights=c["weights"].to(dev))))


def test_j_image_metrics_with_weights_is_out6_and_without_is_todays_call(gpu_device):
    dev = gpu_device
    c = Q.case("noise", (3, 33, 55), 0.2, "frame", None)
    img, gt, w = c["img"].to(dev), c["gt"].to(dev), c["weights"].to(dev)
    out6, _, _ = _run(c, dev, want_grad=False)
    totals = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=dev)
    m = G.image_metrics(img, gt, weights=w, totals=totals)
    assert torch.equal(_bits(m), _bits(out6[[5, 2, 1, 4]]))
    assert totals.cpu().tolist() == [1.0 + float(m[0]), 2.0 + float(m[1]), 3.0 + float(m[2]), 5.0]
    _hold(c, out6, None, None, "image_metrics, weights")
    # without weights: the call as it was, bit for bit (the C entry point directly)
    L = G._capi.lib()
    nbytes = int(L.gsr_image_metrics_workspace(3, 33, 55))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out4 = torch.empty(4, device=dev)
    win = (C.c_float * 11)(*c["win"].tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.gsr_image_metrics(3, 33, 55, img.data_ptr(), gt.data_ptr(), win, out4.data_ptr(), None, ws.data_ptr(), nbytes, stream) == 0
    assert torch.equal(_bits(G.image_metrics(img, gt)), _bits(out4))
    # a frame charges the plain PSNR for its black border; the weighted one is not charged
    dark = c["img"].clone() * c["weights"]
    plain, fair = G.image_metrics(dark.to(dev), gt), G.image_metrics(dark.to(dev), gt, weights=w)
    assert float(fair[0]) > float(plain[0])


# ---- (k) buffers: through the C ABI, every buffer a view at a chosen byte offset inside a NaN-patterned allocation ----
def _written(t):
    return not bool((t.view(torch.int32) == A.PAT).any())


@pytest.mark.parametrize("mode", ["a0", "a4", "a8", "a12", "mix"])
@pytest.mark.parametrize("key", [("edges", (3, 33, 55), 0.2, "gate", "rows"), ("noise", (1, 65, 109), 0.2, "ramp", None)],
                         ids=IDS)
def test_k_misaligned_guarded_buffers_and_an_exact_workspace(key, mode, gpu_device):
    dev = gpu_device
    c = Q.case(*key)
    L = G._capi.lib()
    Cn, H, W = shape = tuple(c["img"].shape)
    nbytes = int(L.gsr_weighted_loss_workspace(Cn, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    ar = A.Arena(dev, A.offsets(mode))
    ar.put("img", c["img"]), ar.put("gt", c["gt"]), ar.put("weights", c["weights"])
    if c["acc"] is not None:
        ar.put("acc", c["acc"])
    if c["e"] is not None:
        ar.put("e", c["e"]), ar.put("dexp", shape=(Cn, 2))
    ar.put("out6", shape=(6,)), ar.put("dimg", shape=shape)
    ar.put("ws", shape=(nbytes // 4,))                           # EXACTLY the bytes asked for
    opt = lambda k: ar.ptr(k) if k in ar.t else None  # noqa: E731
    win = (C.c_float * 11)(*c["win"].tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = _run(c, dev)
    for want_grad in (True, False):
        code = L.gsr_weighted_loss(*shape, ar.ptr("img"), ar.ptr("gt"), ar.ptr("weights"), opt("acc"),
                                   C.c_float(Q.ACC_MIN), opt("e"), win, C.c_float(c["lam"]), ar.ptr("out6"),
                                   ar.ptr("dimg") if want_grad else None, opt("dexp") if want_grad else None,
                                   ar.ptr("ws"), nbytes, stream)
        torch.cuda.synchronize()
        assert code == 0, L.gsr_last_error()
        assert ar.guards_intact() is None, "guard of %s overwritten" % ar.guards_intact()
        assert torch.equal(ar.t["img"].cpu(), c["img"]) and torch.equal(ar.t["weights"].cpu(), c["weights"])
        assert _written(ar.t["out6"]) and torch.equal(_bits(ar.t["out6"]), _bits(ref[0]))
        if want_grad:
            assert _written(ar.t["dimg"]) and torch.equal(_bits(ar.t["dimg"]), _bits(ref[1]))
            if c["e"] is not None:
                assert _written(ar.t["dexp"]) and torch.equal(_bits(ar.t["dexp"]), _bits(ref[2]))
            ar.t["out6"].view(torch.int32).fill_(A.PAT)
    _hold(c, ar.t["out6"], ar.t["dimg"], ar.t["dexp"] if c["e"] is not None else None, "guarded", mode=mode,
          shape=list(shape))


def test_profile_counts_the_launches_under_the_exposure_ids(gpu_device):
    """Forward, backward and finish with the gradients, forward and finish without: the exposure loss's launches."""
    dev = gpu_device
    c = Q.case("noise", (3, 33, 55), 0.2, "ramp", "rows")
    counts = {}
    for want in (True, False):
        _run(c, dev, want)
        G.profile_enable(True)
        try:
            _run(c, dev, want)
            torch.cuda.synchronize()
        finally:
            G.profile_enable(False)
        counts[want] = {k: v[1] for k, v in G.profile_read().items() if v[1]}
    assert counts[True] == dict(k_exposure_loss_forward=1, k_exposure_loss_backward=1, k_exposure_loss_finish=1)
    assert counts[False] == dict(k_exposure_loss_forward=1, k_exposure_loss_finish=1)


# ---- evaluate_keyframes(weights=...) -------------------------------------------------------------------------------
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


def test_evaluate_keyframes_with_weights(gpu_device):
    """Two 48 x 64 keyframes; the second one's ground truth has a black 6-pixel border (an undistorted image).  Without
    its weight map the keyframe is charged for the border; with it the row is image_metrics(weights=) of the render,
    and a keyframe given None keeps today's row."""
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
    border = torch.zeros((H, W), device=dev)
    border[6:H - 6, 6:W - 6] = 1.0
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        with torch.no_grad():
            images = [G.render(c, model, bg)[0] for c in cams]
            gts = [G.render(c, other, bg)[0] for c in cams]
            gts[1] = gts[1] * border
        plain = G.evaluate_keyframes(cams, gts, model, bg)
        fair = G.evaluate_keyframes(cams, gts, model, bg, weights=[None, border])
        with pytest.raises(ValueError):
            G.evaluate_keyframes(cams, gts, model, bg, weights=[border])
    finally:
        G.set_near_far_thread(prev_nf)
    assert torch.equal(_bits(fair["rows"][0]), _bits(plain["rows"][0]))
    assert torch.equal(_bits(fair["rows"][1]), _bits(G.image_metrics(images[1], gts[1], weights=border).cpu()))
    assert float(fair["rows"][1][0]) > float(plain["rows"][1][0]) and fair["frames"] == 2
    want = fair["rows"][:, :3].double().sum(0)
    assert bool(((fair["totals"][:3] - want).abs() <= 1e-12 * want.abs()).all()) and float(fair["totals"][3]) == 2.0
