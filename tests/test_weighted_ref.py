"""CPU tests of tests/weighted_ref.py: the truth the weighted photometric loss (csrc/weighted.hip) is held to is the
definition, its bars are not vacuous, and each of eight wrong definitions is refused by them."""
import json
import math

import pytest
import torch

import exposure_ref as X
import loss_ref as R
import weighted_ref as Q

TINY = [(1, 1, 1), (2, 3, 4), (1, 6, 7)]
IDS = lambda v: str(v).replace(" ", "")  # noqa: E731


def _tiny(shape, pat):
    img, gt = R.make("noise", shape)
    weights, acc = Q.pattern(pat, shape)
    return img, gt, Q.effective(weights, acc, Q.ACC_MIN, shape)


@pytest.mark.parametrize("shape", TINY, ids=IDS)
@pytest.mark.parametrize("pat", ["ramp", "gate", "corner"])
def test_conv2d_truth_equals_the_loop_over_pixels_and_taps(shape, pat):
    img, gt, w = _tiny(shape, pat)
    win = R.reference_window_1d()
    for lam in R.LAMS:
        a, b = Q.parts(img, gt, w, win, lam, torch.float64), Q.parts_definition(img, gt, w, win, lam)
        for k in ("loss", "l1", "ssim", "S", "mse"):
            assert abs(a[k] - b[k]) <= 1e-13 * max(1.0, abs(b[k])), (k, a[k], b[k])
        assert bool(((a["grad"] - b["grad"]).abs() <= 1e-13 * (1 + b["grad"].abs())).all())


@pytest.mark.parametrize("shape", [(3, 7, 5), (3, 33, 55)], ids=IDS)
def test_with_ones_it_is_loss_ref_and_exposure_ref(shape):
    img, gt = R.make("edges", shape)
    win, ones = R.reference_window_1d(), torch.ones(shape[1:])
    for lam in R.LAMS:
        for dtype in (torch.float64, torch.float32):
            a, b = Q.parts(img, gt, ones, win, lam, dtype), R.loss_parts(img, gt, win, lam, dtype)
            tol = 1e-13 if dtype == torch.float64 else 1e-5
            for k in ("loss", "l1", "ssim"):
                assert abs(a[k] - b[k]) <= tol * max(1.0, abs(b[k])), (k, dtype)
            assert bool(((a["grad"] - b["grad"]).abs() <= tol * (1e-3 + b["grad"].abs())).all())
        e = X.exposure("negative", shape[0])
        t, u = Q.truth(img, gt, e, None, None, Q.ACC_MIN, win, lam), X.truth(img, gt, e, win, lam)
        assert bool(((t["dimg"] - u["dimg"]).abs() <= 1e-13 * (1e-3 + u["dimg"].abs())).all())
        assert bool(((t["dexp"] - u["dexp"]).abs() <= 1e-12 * (1e-3 + u["dexp"].abs())).all())
        assert t["r64"]["S"] == shape[1] * shape[2]
        # the weighted floors are loss_ref's with the larger counts: never below them, and by no more than the counts say
        fq, fr = Q.floors(t["xp"], gt, ones, win, lam), R.floors(t["xp"], gt, win, lam)
        ratio = fq["grad"] / fr["grad"].clamp(min=1e-300)
        assert bool(((ratio - Q.K["grad"] / R.K["grad"]).abs() <= 1e-9)[fr["grad"] > 0].all())
        assert fr["l1"] <= fq["l1"] <= 2 * fr["l1"] and fr["ssim"] <= fq["ssim"] <= 2 * fr["ssim"]


def test_gradcheck_in_float64_and_the_floor_formula():
    shape = (2, 6, 7)
    img, gt, w = _tiny(shape, "ramp")
    win = R.reference_window_1d()
    y, ww = gt.double(), w.double()

    def f(x):
        sv = Q.ssim_map(x, y, win)
        n = shape[0] * ww.sum()
        return 0.8 * (ww * (x - y).abs()).sum() / n + 0.2 * (1 - (ww * sv).sum() / n)

    x = (img.double() + 0.01).requires_grad_(True)          # (no pixel at x == y: |.| is smooth there)
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    for lam in R.LAMS:
        g = Q.parts(img, gt, w, win, lam, torch.float64)["grad"]
        formula = Q.floors(img, gt, w, win, lam)["formula_grad"]
        assert bool(((g - formula).abs() <= 1e-12 * (1e-3 + g.abs())).all())


@pytest.mark.parametrize("pat", ["frame", "ramp", "gate"])
def test_scaling_the_weights_changes_only_S(pat):
    shape = (3, 33, 55)
    img, gt = R.make("noise", shape)
    weights, acc = Q.pattern(pat, shape)
    win = R.reference_window_1d()
    base = Q.parts(img, gt, Q.effective(weights, acc, Q.ACC_MIN, shape), win, 0.2, torch.float64)
    for s in (4.0, 0.125) + ((3.0,) if pat == "frame" else ()):      # (3 w is exact in float32 for a {0, 1} map only)
        r = Q.parts(img, gt, Q.effective(weights * s, acc, Q.ACC_MIN, shape), win, 0.2, torch.float64)
        tol = 0.0 if s != 3.0 else 1e-14
        for k in ("loss", "l1", "ssim", "mse", "psnr"):
            assert abs(r[k] - base[k]) <= tol * abs(base[k]), (k, s)
        assert abs(r["S"] - s * base["S"]) <= tol * r["S"]
        assert bool(((r["grad"] - base["grad"]).abs() <= tol * base["grad"].abs().max()).all())


def test_every_pattern_but_zero_supervises_something_and_no_input_has_an_fma_tie():
    for shape in Q.SHAPES + [Q.MANY]:
        for pat in Q.PATTERNS:
            weights, acc = Q.pattern(pat, shape)
            w = Q.effective(weights, acc, Q.ACC_MIN, shape)
            assert bool(torch.isfinite(w).all()) and bool((w >= 0).all())
            assert (float(w.sum()) > 0) == (pat != "zero"), (shape, pat)
        for gen in X.GENS:
            img, _ = R.make(gen, shape)
            for ek in Q.EXPOSURES[1:]:
                assert X.ties(img, Q.exposure(ek, shape[0])) == 0, (gen, shape, ek)
    weights, acc = Q.pattern("gate", (3, 33, 55))
    w = Q.effective(weights, acc, Q.ACC_MIN, (3, 33, 55))
    at, nan = acc == 0.5, torch.isnan(acc)
    assert bool(at.any()) and int(nan.sum()) == 1 and bool((acc < 0.5).any()) and bool((acc > 0.5).any())
    assert bool((w[at] == weights[at]).all()) and float(w[nan]) == 0.0 and bool((w[acc < 0.5] == 0).all())
    assert bool((weights[nan] > 0).all()) and bool((weights[at] > 0).any())      # (so both gate mutants change S)


@pytest.mark.parametrize("name,shape,lam,pat,ekey", Q.CASES, ids=IDS)
def test_float32_in_the_kernels_order_is_inside_every_bar(name, shape, lam, pat, ekey):
    """The separable float32 evaluation (two 11-tap passes, the variances through win(xx + yy)) is not the one e_ref
    was taken from, and is held at the very bars the kernels are held at."""
    c = Q.case(name, shape, lam, pat, ekey)
    r = Q.parts(c["xp"], c["gt"], c["w"], c["win"], lam, torch.float32, separable=True)
    dimg, dexp = Q.closed_forms(r["grad"], c["img"], c["e"])
    res = Q.ratios(c, [r[k] for k in Q.SCALARS], dimg, dexp)
    assert all(v <= 1.0 for v in res.values()), res
    if pat == "zero":
        assert c["r64"]["S"] == 0 and c["r64"]["psnr"] == math.inf and not bool(c["dimg"].any())


# ---- the mutants: (mutant, case, the outputs the float64 check at the bars refuses it on) ----------------------------
MUTANT_CASES = [
    ("norm_hw", ("noise", (3, 33, 55), 0.2, "frame", "rows")),
    ("mask_images", ("noise", (3, 33, 55), 0.2, "frame", "rows")),
    ("l1_grad_without_w", ("noise", (3, 33, 55), 0.2, "ramp", None)),
    ("maps_without_w", ("noise", (3, 33, 55), 0.2, "ramp", None)),
    ("gate_gt", ("noise", (3, 33, 55), 0.2, "gate", "rows")),
    ("gate_lets_nan", ("noise", (3, 33, 55), 0.2, "gate", "rows")),
    ("s_all_channels", ("noise", (3, 33, 55), 0.2, "ramp", "negative")),
    ("pad_with_bias", ("noise", (3, 33, 55), 0.2, "ones", "negative")),
]


def mutant_table():
    rows = []
    for name, key in MUTANT_CASES:
        c = Q.case(*key)
        out6, dimg, dexp = Q.mutant(name, c["img"], c["gt"], c["e"], c["weights"], c["acc"], Q.ACC_MIN, c["win"], c["lam"])
        res = Q.ratios(c, out6, dimg, dexp)
        rows.append(dict(mutant=name, case=list(key), over_bar={k: float("%.4g" % v) for k, v in res.items()}))
    return rows


def test_every_mutant_of_the_definition_is_refused_at_the_bars():
    assert [m for m, _ in MUTANT_CASES] == list(Q.MUTANTS)
    for row in mutant_table():
        print(json.dumps(row))
        r = row["over_bar"]
        assert max(r.values()) > 1.0, row                       # test_gpu_weighted's float64 check refuses it
        if row["mutant"] in ("norm_hw", "s_all_channels", "mask_images"):
            assert r["loss"] > 1.0 and r["dimg"] > 1.0, row     # a wrong normaliser shows in every normalised number
        if row["mutant"] in ("gate_gt", "gate_lets_nan"):
            assert r["S"] > 1.0, row                            # the supervised set itself differs
        if row["mutant"] in ("l1_grad_without_w", "maps_without_w"):
            assert r["loss"] == 0.0 and r["dimg"] > 1.0, row    # the values are right, only the gradient is not
        if row["mutant"] == "pad_with_bias":
            assert r["ssim"] > 1.0 and r["l1"] == 0.0, row      # only the windows at the border see the padding
