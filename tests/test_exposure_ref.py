"""CPU tests of tests/exposure_ref.py itself: the restated FMA is the FMA, the closed forms are autograd's, the bars
admit a float32 evaluation of the whole chain and refuse the padding mistake."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import exposure_ref as X
import loss_ref as R


def test_no_element_of_the_cases_sits_on_a_double_rounding_tie():
    for name, shape, _, ekey in X.CASES:
        img, _ = R.make(name, shape)
        assert X.ties(img, X.exposure(ekey, shape[0])) == 0, (name, shape, ekey)
    # the detector sees one: (1 + 2^-23) * 2^-24 (1 - 2^-23) + 1 = 1 + 2^-24 - 2^-70 is rounded, in float64, onto the
    # midpoint 1 + 2^-24; the exact midpoint 1 * 2^-24 + 1 is no hazard
    assert X.ties(torch.tensor([[[2.0 ** -24 * (1 - 2.0 ** -23)]]]), torch.tensor([[1.0 + 2.0 ** -23, 1.0]])) == 1
    assert X.ties(torch.tensor([[[2.0 ** -24]]]), torch.tensor([[1.0, 1.0]])) == 0


def test_compensate_is_the_correctly_rounded_fma_in_exact_rationals():
    """Every element of one small case: no float32 value is nearer to the exact rational g x + b than the one returned
    (with no tie, that is the FMA's result)."""
    for ekey in ("rows", "negative"):
        img, _ = R.make("noise", (3, 7, 5))
        e = X.exposure(ekey, 3)
        got = X.compensate(img, e).numpy()
        for c in range(3):
            g, b = Fraction(float(e[c, 0])), Fraction(float(e[c, 1]))
            for x, v in zip(img[c].reshape(-1).tolist(), got[c].reshape(-1)):
                exact = g * Fraction(x) + b
                err = abs(Fraction(float(v)) - exact)
                for nb in (np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))):
                    other = abs(Fraction(float(nb)) - exact)
                    # (an exact tie -- g = 1.25 has three bits -- goes to the even mantissa, as the FMA's does)
                    assert err < other or (err == other and int(v.view(np.int32)) % 2 == 0), (c, x, v)
    ident = X.compensate(img, X.exposure("identity", 3))
    assert torch.equal(ident.view(torch.int32), img.view(torch.int32))   # (no negative zero among these inputs)


def test_loss64_is_loss_parts_and_autograd_agrees_with_the_closed_forms():
    for name, shape, lam, ekey in (("noise", (3, 7, 5), 0.2, "rows"), ("edges", (3, 33, 55), 1.0, "negative"),
                                   ("bright", (1, 65, 109), 0.0, "rolled")):
        c = X.case(name, shape, lam, ekey)
        x = c["img"].double().requires_grad_(True)
        e = c["e"].double().requires_grad_(True)
        out = X.loss64(e[:, 0, None, None] * x + e[:, 1, None, None], c["gt"].double(), c["w"], lam)
        gx, ge = torch.autograd.grad(out["loss"], (x, e))
        # (x' differs from compensate's by the float32 rounding of the FMA: 2^-24 relative, in a float64 evaluation)
        for k in ("loss", "l1", "ssim"):
            assert abs(float(out[k].detach()) - c["r64"][k]) <= 1e-6 * max(1.0, abs(c["r64"][k])), k
        at_xp = X.loss64(c["xp"].double().requires_grad_(True), c["gt"].double(), c["w"], lam)
        for k in ("loss", "l1", "ssim"):
            assert abs(float(at_xp[k].detach()) - c["r64"][k]) <= 1e-12, k
        scale = float(c["dimg"].abs().max())
        assert float((gx - c["dimg"]).abs().max()) <= 1e-5 * scale
        assert float((ge - c["dexp"]).abs().max()) <= 1e-5 * float(c["dexp"].abs().max())


def test_gradcheck_through_the_compensation():
    img, gt = R.make("noise", (3, 7, 5))
    w = R.reference_window_1d()
    x = img.double().requires_grad_(True)
    e = X.exposure("rows", 3).double().requires_grad_(True)
    f = lambda x, e: X.loss64(e[:, 0, None, None] * x + e[:, 1, None, None], gt.double(), w, 0.2)["loss"]  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, e), eps=1e-7, atol=1e-8, rtol=1e-5)


@pytest.mark.parametrize("name,shape,lam,ekey", [c for c in X.CASES if c[1] != X.MANY][::3] + [X.CASES[-1]],
                         ids=lambda v: str(v).replace(" ", ""))
def test_a_float32_restatement_of_the_whole_chain_lies_inside_every_bar(name, shape, lam, ekey):
    """The bars are not vacuous: float32 evaluations of the chain -- loss_ref's two (conv2d; separable, four moments),
    the product with g in float32, the two sums narrowed once -- pass them."""
    c = X.case(name, shape, lam, ekey)
    g32 = c["e"][:, 0, None, None]
    for sep in (False, True):
        r = R.loss_parts(c["xp"], c["gt"], c["w"], lam, torch.float32, separable=sep)
        G = r["grad"].float()
        dimg = g32 * G
        dexp = torch.stack(((G.double() * c["img"].double()).sum((1, 2)), G.double().sum((1, 2))), dim=1).float()
        res = X.ratios(c, (r["loss"], r["l1"], r["ssim"]), dimg, dexp)
        assert all(v <= 1.0 for v in res.values()), (sep, res)


def test_mistakes_restated_in_float64_leave_the_bars():
    """The mistakes a kernel of this kind can make, each restated on the truth's own float64 numbers (no kernel is
    built wrong): what the GPU tests compare -- X.ratios over all elements -- refuses every one of them but the last."""
    c = X.case("noise", (3, 33, 55), 0.2, "rows")
    G, x, e = c["r64"]["grad"], c["img"].double(), c["e"]
    dimg, dexp = X.closed_forms(G, c["img"], e)
    over = lambda **kw: X.ratios(c, **kw)  # noqa: E731
    # x' for x in sum G x
    wrong = dexp.clone()
    wrong[:, 0] = (G * c["xp"].double()).sum((1, 2))
    assert over(dexp=wrong)["dexp"] > 1.0
    # dL/dimg without g
    assert over(dimg=G)["dimg"] > 1.0
    # exposure[c] read for the wrong channel
    t = X.truth(c["img"], c["gt"], e.roll(1, 0), c["w"], 0.2)
    res = over(out3=(t["r64"]["loss"], t["r64"]["l1"], t["r64"]["ssim"]), dimg=t["dimg"], dexp=t["dexp"])
    assert all(v > 1.0 for v in res.values()), res
    # the last work unit's pair dropped (the 1 x 1 pixel corner unit of a 33 x 55 plane)
    wrong = dexp.clone()
    wrong[:, 0] -= G[:, 32:, 54:].sum((1, 2)) * x[:, 32, 54]
    wrong[:, 1] -= G[:, 32:, 54:].sum((1, 2))
    assert over(dexp=wrong)["dexp"] > 1.0
    # sum G without the L1 term
    lam = R.lam32(0.2)
    ssim_only = G - (1 - lam) / G.numel() * torch.sign(c["xp"].double() - c["gt"].double())
    assert over(dexp=X.closed_forms(ssim_only, c["img"], e)[1])["dexp"] > 1.0
    # float32 partial sums per work unit: SURVIVES -- the bars of the two sums are worst-case sums of bar_G, thousands
    # of times the rounding of a float32 sum of 1728 terms
    f32 = torch.stack(((G * x).float().sum((1, 2), dtype=torch.float32), G.float().sum((1, 2), dtype=torch.float32)), 1)
    assert over(dexp=f32)["dexp"] <= 1.0


def test_padding_with_b_is_refused_at_a_border_pixel():
    """x' formed behind the padding select pads with b_c.  At b != 0 the mutant's gradient leaves the bar at a border
    pixel, its SSIM leaves the scalar's bar and both exposure gradients leave theirs."""
    c = X.case("noise", (3, 33, 55), 1.0, "rows")
    xp = c["xp"].double().requires_grad_(True)
    out = X.loss64(xp, c["gt"].double(), c["w"], 1.0, pad_value=c["e"][:, 1].double())
    (G,) = torch.autograd.grad(out["loss"], xp)
    dimg, dexp = X.closed_forms(G, c["img"], c["e"])
    over = (dimg - c["dimg"]).abs() / c["bar_dimg"]
    border = torch.zeros(c["img"].shape[1:], dtype=torch.bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    assert float(over[0][border].max()) > 1.0 and float(over[2][border].max()) > 1.0   # b = -0.05 and 0.1
    assert float(over[1].max()) <= 1e-6                                                 # b = 0: the same function
    assert float(over[0][16, 27]) <= 1.0                                                # and far from the border
    assert abs(float(out["ssim"].detach()) - c["r64"]["ssim"]) > c["bar"]["ssim"][1]
    assert bool(((dexp - c["dexp"]).abs()[[0, 2]] > c["bar_dexp"][[0, 2]]).all())
