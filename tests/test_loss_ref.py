"""CPU anchor of tests/loss_ref.py, the float64 reference csrc/loss.hip is held to (test_gpu_loss_ref64.py): the conv2d
restatement against the definition written as loops, gradcheck, the closed form of an impulse's SSIM gradient, and the
bars exercised on the float32 / float64 pair of the restatement itself on every input the GPU module uses."""
import json

import pytest
import torch

import loss_ref as R

U64 = 2.0 ** -52


def test_window_is_the_packages():
    from gs_livm_amd.loss import reference_window_1d
    assert torch.equal(R.reference_window_1d(), reference_window_1d())
    w = R.reference_window_1d()
    assert not torch.equal(w, w.flip(0))  # asymmetric: orientation matters


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 13), (3, 12, 7)])
@pytest.mark.parametrize("window", ["reference", "symmetric"])
def test_conv2d_restatement_equals_the_definition(shape, window):
    """Float64 conv2d against the loop over pixels and taps: same values up to the order of a 121-term sum
    (121 float64 roundings of the sum of absolute terms <= 1 for SSIM, <= 1 / N a pixel for the gradient; 1e-13 is
    generous by 4 decades and 8 decades below any wrong tap)."""
    w = R.reference_window_1d() if window == "reference" else R.symmetric_window_1d()
    for gen, lam in ((R.noise, 0.2), (R.edges, 1.0), (R.bright, 0.0)):
        img, gt = gen(shape)
        a, b = R.loss_parts(img, gt, w, lam, torch.float64), R.loss_parts_definition(img, gt, w, lam)
        for k in ("loss", "l1", "ssim"):
            assert abs(a[k] - b[k]) <= 1e-13 * max(1.0, abs(b[k])), (k, a[k], b[k])
        assert float((a["grad"] - b["grad"]).abs().max()) <= 1e-13 * max(1.0, float(b["grad"].abs().max()))
        f = R.floors(img, gt, w, lam)   # the maps A, B, C the floors are built from give the same gradient
        assert float((f["formula_grad"] - b["grad"]).abs().max()) <= 1e-13 * max(1.0, float(b["grad"].abs().max()))


def test_definition_distinguishes_the_window_orientation():
    """With the flipped window the definition gives another loss: the asymmetry is large enough to see (> 1e-4)."""
    img, gt = R.noise((1, 12, 13))
    w = R.reference_window_1d()
    a, b = R.loss_parts_definition(img, gt, w, 1.0), R.loss_parts_definition(img, gt, w.flip(0), 1.0)
    assert abs(a["ssim"] - b["ssim"]) > 1e-4


def test_gradcheck_and_sign_of_zero():
    img, gt = R.noise((2, 5, 7))
    d = img - gt
    img = gt + torch.where(d >= 0, d.clamp(min=0.01), d.clamp(max=-0.01))   # no ties, none within gradcheck's step
    assert float((img - gt).abs().min()) > 1e-3
    w = R.reference_window_1d().double()

    def f(x, lam):
        ch = x.shape[0]
        window = R._window(w, ch)
        conv = lambda t: torch.nn.functional.conv2d(t[None], window, padding=5, groups=ch)[0]  # noqa: E731
        y = gt.double()
        mu1, mu2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
        m = ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s1 + s2 + R.C2))
        return (1 - lam) * (x - y).abs().mean() + lam * (1 - m.mean())

    for lam in (0.0, 0.25, 1.0):
        x = img.double().clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: f(t, lam), (x,), eps=1e-7, atol=1e-7, rtol=1e-5)
        got = R.loss_parts(img, gt, R.reference_window_1d(), lam, torch.float64)
        (want,) = torch.autograd.grad(f(x, R.lam32(lam)), x)
        assert float((got["grad"] - want).abs().max()) <= 64 * U64 * float(want.abs().max())  # the same function
    # abs'(0) = 0: with img == gt and lam = 0 the gradient is exactly zero, in both dtypes
    for dt in (torch.float64, torch.float32):
        r = R.loss_parts(gt, gt, R.reference_window_1d(), 0.0, dt)
        assert r["loss"] == 0.0 and not bool(r["grad"].any())


@pytest.mark.parametrize("shape,py,px", [((1, 14, 15), 0, 0), ((2, 14, 15), 13, 14), ((1, 14, 15), 0, 7),
                                         ((1, 14, 15), 6, 14), ((1, 14, 15), 7, 6), ((1, 3, 4), 1, 2), ((1, 1, 1), 0, 0)])
def test_impulse_gradient_has_its_closed_form(shape, py, px):
    """An impulse against a zero target: the SSIM gradient from the taps alone (impulse_ssim_gradient) against the
    restatement's autograd, for both windows.  Bar: 1e-12 of the largest gradient element (float64 sums of <= 121 terms;
    a wrong tap or a missing pad moves it by parts in ten)."""
    for w in (R.reference_window_1d(), R.symmetric_window_1d()):
        for amp in (1.0, 0.05):
            img, gt = R.impulse(shape, py, px, 0.0, amp)
            got = R.loss_parts(img, gt, w, 1.0, torch.float64)["grad"]      # lam = 1: d(1 - ssim) / dimg
            want = -R.impulse_ssim_gradient(shape, py, px, float(img[0, py, px]), w)   # (the float32 value of amp)
            scale = float(want.abs().max())
            assert scale > 0 and float((got - want).abs().max()) <= 1e-12 * scale
            touched = got != 0
            ys, xs = torch.nonzero(touched.any(0), as_tuple=True)
            assert int(ys.min()) >= py - 10 and int(ys.max()) <= py + 10 and int(xs.min()) >= px - 10 and int(xs.max()) <= px + 10


SCALARS = ("loss", "l1", "ssim")
ALL_CASES = [("gen",) + c for c in R.CASES] + [("impulse",) + c for c in R.impulse_cases()]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "-".join(str(v).replace(" ", "") for v in c))
def test_float32_evaluations_stay_inside_the_bars_on_every_gpu_case(case):
    """What the reference alone must pass, on every input of test_gpu_loss_ref64.py: finite, d2 > 0; the three scalars
    of the float32 restatement inside the FLOORS alone (no 2 e_ref: that would be vacuous); and a second float32
    evaluation in another order of operations (separable passes, four moments) inside every bar, the per-pixel
    gradient bars included -- a float32 evaluation the bars were not taken from."""
    c = R.case(*case[1:]) if case[0] == "gen" else R.impulse_case(*case[1:])
    r64, r32, fl = c["r64"], c["r32"], c["floors"]
    assert r32["d2_min"] > 0 and r64["d2_min"] > 0, r32["d2_min"]
    assert bool(torch.isfinite(r32["grad"]).all()) and bool(torch.isfinite(r64["grad"]).all())
    for k, (e, b) in c["bar"].items():
        assert bool(torch.as_tensor(b >= 2 * e).all()) and bool(torch.as_tensor(b >= fl[k]).all())
    own = {k: abs(r32[k] - r64[k]) / fl[k] for k in SCALARS}
    sep = R.loss_parts(c["img"], c["gt"], c["w"], c["lam"], torch.float32, separable=True)
    res = {k: v[3] for k, v in R.worst_ratios(sep, r64, c["bar"]).items()}
    e = (r32["grad"] - r64["grad"]).abs()
    over = torch.where(fl["grad"] > 0, e / fl["grad"].clamp(min=1e-300), torch.zeros_like(e))
    print(json.dumps(dict(what="float32 on the CPU", case=[str(v) for v in case[1:]],
                          restatement_over_floor={k: float("%.3g" % v) for k, v in own.items()},
                          restatement_grad_over_count_only_floor=float("%.3g" % float(over.max())),
                          separable_over_bar={k: float("%.3g" % v) for k, v in res.items()})))
    for k, v in own.items():
        assert v <= 1.0, "%s: float32 Torch is at %.3g of the floor" % (k, v)
    for k, v in res.items():
        assert v <= 1.0, "%s: the separable float32 evaluation is at %.3g of the bar" % (k, v)


def test_amplitude_walk_behind_the_cap_of_bright():
    """The walk quoted in loss_ref.py: the scalars on noise and edges inside the floors up to 256; constant planes keep
    the float32 restatement's d2 positive up to 32 and lose it by 48."""
    w = R.reference_window_1d()
    shape = (3, 38, 60)
    for gen in (R.noise, R.edges):
        for a in (R.BRIGHT_AMPLITUDE, 32.0, 256.0):
            img, gt = gen(shape, 0, a)
            r64, r32 = R.loss_parts(img, gt, w, 1.0, torch.float64), R.loss_parts(img, gt, w, 1.0, torch.float32)
            fl = R.floors(img, gt, w, 1.0)
            res = {k: abs(r32[k] - r64[k]) / fl[k] for k in SCALARS}
            assert r32["d2_min"] > 0 and bool(torch.isfinite(r32["grad"]).all()), (gen.__name__, a)
            assert all(v <= 1.0 for v in res.values()), (gen.__name__, a, res)
    d2 = {}
    for a in (R.BRIGHT_AMPLITUDE, 32.0, 48.0):
        img, gt = torch.full(shape, a), torch.full(shape, 0.75 * a)
        d2[a] = R.loss_parts(img, gt, w, 1.0, torch.float32, want_grad=False)["d2_min"]
    print(json.dumps(dict(what="smallest float32 d2 on constant planes", d2=d2)))
    assert d2[R.BRIGHT_AMPLITUDE] > 0.98 * R.C2 and d2[32.0] > 0 and d2[48.0] <= 0


def test_generators_deliver_what_they_promise():
    s = (3, 38, 60)
    img, gt = R.dark(s)
    assert float(img.max()) <= 0.02 and float(gt.max()) <= 0.02
    img, gt = R.bright(s)
    assert 3.5 < float(img.max()) <= R.BRIGHT_AMPLITUDE
    img, gt = R.equal_but_one(s)
    assert int((img != gt).sum()) == 1 and bool((img != gt)[R.one_pixel(s)])
    img, gt = R.edges(s)
    flat = (img[:, :, 1:] == img[:, :, :-1]).float().mean()
    assert 0.85 < float(flat) < 1.0 and img.unique().numel() <= 3 * 8 * 7
    img, gt = R.impulse(s, 37, 59, 0.5)
    assert int((img != 0).sum()) == 3 and bool((gt == 0.5).all())
    shapes = {c[1] for c in R.CASES}
    assert set(R.SEAM_SHAPES) | set(R.MANY_PARTIALS) <= shapes
    for name in R.GENERATORS:
        assert {lam for g, _, lam in R.CASES if g == name} == set(R.LAMS)
