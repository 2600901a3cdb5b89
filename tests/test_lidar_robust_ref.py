"""CPU tests of tests/lidar_robust_ref.py, the restatement tests/test_gpu_lidar_robust.py holds csrc/lidar.hip's
occlusion filter and robust depth loss to: the Torch-op filter equals the loop exactly, the float32 restatement of the
loss stays inside the bars on every GPU-test input, those inputs hold no clip-fragile pixel, the F3 share stays under
1 %, every branch is occupied, and the float64 loss at the identity parameters is lidar_ref.loss_ops exactly."""
import numpy as np
import pytest
import torch

import lidar_ref as L
import lidar_robust_ref as R

F64 = torch.float64
SHAPES = ((1, 1), (3, 5), (37, 61), (70, 130))


@pytest.mark.parametrize("shape", SHAPES)
def test_filter_ops_equals_the_loop(shape):
    img = R.filter_image(*shape)
    for radius in (0, 1, 2, 3):
        for tol in (0.0, 0.05):
            want, kept, removed = R.filter32(img, radius, tol)
            got = R.filter_ops(torch.from_numpy(img), radius, tol).numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (radius, tol)
            with np.errstate(invalid="ignore"):
                assert kept + removed == int((img > 0).sum()) and kept == int((want > 0).sum())


def test_filter_ops_equals_the_loop_at_512x640():
    img = R.filter_image(512, 640)
    want, kept, removed = R.filter32(img, 3, 0.05)
    got = R.filter_ops(torch.from_numpy(img), 3, 0.05).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and removed > 1000 and kept > 1000


def test_filter_closed_forms():
    """radius 0 cleans and copies; a return behind a nearer one goes, the nearer one stays; a difference of exactly
    tol * z stays (the rule is >); the window is clamped (a corner pixel sees its three neighbours); zeros, negatives and
    NaN never serve as the minimum; +inf is a return that nothing removes at tol > 0 and that removes nothing."""
    img = R.filter_image(37, 61)
    out, kept, removed = R.filter32(img, 0, 0.05)
    with np.errstate(invalid="ignore"):
        assert removed == 0 and np.array_equal(out.view(np.int32), np.where(img > 0, img, np.float32(0)).view(np.int32))
    z = np.zeros((5, 5), np.float32)
    z[2, 2], z[2, 3] = 2.0, 8.0
    out, kept, removed = R.filter32(z, 1, 0.05)
    assert (kept, removed) == (1, 1) and out[2, 2] == 2.0 and out[2, 3] == 0.0
    assert R.filter32(z, 0, 0.05)[2] == 0 and R.filter32(z, 1, 0.75)[2] == 0      # 8 - 2 == 0.75 * 8: kept
    assert R.filter32(z, 1, float(np.nextafter(np.float32(0.75), np.float32(0))))[2] == 1
    z[2, 2] = 0.0
    z[0, 0], z[1, 1], z[4, 4], z[3, 3] = 8.0, 2.0, 8.0, -2.0
    out = R.filter32(z, 1, 0.05)[0]
    assert out[0, 0] == 0.0 and out[1, 1] == 2.0 and out[4, 4] == 8.0 and out[3, 3] == 0.0
    z[3, 3], z[2, 3] = np.nan, np.inf
    out = R.filter32(z, 3, 0.05)[0]
    assert out[3, 3] == 0.0 and out[2, 3] == np.inf and out[1, 1] == 2.0 and out[4, 4] == 0.0
    assert np.array_equal(R.filter_ops(torch.from_numpy(z), 3, 0.05).numpy().view(np.int32), out.view(np.int32))


def test_filter_image_holds_what_it_claims():
    img = R.filter_image(70, 130)
    with np.errstate(invalid="ignore"):
        assert (img == 0).any() and (img < 0).any() and np.isnan(img).any() and np.isinf(img).any()
    x0, y0 = R.TILE_W, R.TILE_H
    lone = ((y0 + 4, x0 - 1), (y0 + 9, x0 + R.TILE_W), (y0 - 1, x0 + 30), (y0 + R.TILE_H, x0 + 45))
    out = R.filter32(img, 1, 0.05)[0]
    for (y, x), (dy, dx) in zip(lone, ((0, 1), (0, -1), (1, 0), (-1, 0))):
        assert img[y, x] == 1.0 and out[y, x] == 1.0
        assert img[y + dy, x + dx] > 6.0 and out[y + dy, x + dx] == 0.0      # removed inside the tile, through the halo


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_float32_restatement_and_fragile_sets_on_gpu_inputs(case):
    x, ref = R.inputs(case), R.reference(case)
    N = x["H"] * x["W"]
    r = R.loss_ratios({k: ref["f32"][k].to(F64) for k in R.KEYS}, ref)
    print(case, "candidates", ref["n_cand"], "quadratic", ref["n_quad"], "linear", ref["n_lin"], "clipped", ref["n_clip"],
          "F3 %.4f" % (ref["fragile_pixels"] / N), "float32 |d| / bar:", {k: round(v, 3) for k, v in r.items()})
    assert ref["clip_fragile"] == 0
    assert ref["fragile_pixels"] / N <= 0.01
    assert max(r.values()) <= 1.0, r
    # branch occupancy: more than one pixel in each of the three (the single pixel of 1x1 and the empty sweep of
    # 3x5_n0, which has no candidate at all, cannot)
    if N > 1 and x["n"] > 0:
        assert min(ref["n_quad"], ref["n_lin"], ref["n_clip"]) > 1
    assert ref["n_quad"] + ref["n_lin"] == ref["n_sup"] and ref["n_sup"] + ref["n_clip"] == ref["n_cand"]
    # the inputs are lidar_ref's except for the pixels pushed off their clip; lidar_ref's own arrays are untouched
    src = L.inputs(case)
    assert np.array_equal(x["acc"], src["acc"]) and np.array_equal(x["lidar"], src["lidar"])
    assert int((x["depth"] != src["depth"]).sum()) <= 0.05 * N + 1
    t = ref["terms"]
    if ref["n_cand"]:
        assert float((t["a"] - t["clip"]).abs()[t["cand"]].min()) >= 0.5 * R.CLIP_MARGIN


@pytest.mark.parametrize("case", L.CASE_NAMES)
def test_identity_parameters_are_the_plain_loss_exactly(case):
    x = L.inputs(case)
    args = (x["depth"], x["acc"], x["lidar"], x["acc_min"], x["lam"])
    want = L.loss_ops(*args)
    got = R.robust_ops(*args, **R.IDENTITY)
    for k in ("loss", "mean", "share", "grad_depth", "grad_acc"):
        assert torch.equal(got[k], want[k]), k
    assert float(got["clip_share"]) == 0.0


def test_gradient_closed_form():
    """autograd's gradient is c psi / A and -c psi D / A^2 with psi = e / tau inside tau and sign(e) outside"""
    x, ref = R.inputs("37x61_n257"), R.reference("37x61_n257")
    t, tr = ref["terms"], ref["truth"]
    c = x["lam"] / ref["n_sup"]
    gd = torch.where(t["sup"], c * t["psi"] / t["A"], torch.zeros_like(t["A"]))
    assert float((tr["grad_depth"] - gd).abs().max()) <= 1e-15
    assert float((tr["grad_acc"] + gd * t["q"]).abs().max()) <= 1e-14
    assert float(tr["loss"]) == pytest.approx(x["lam"] * float(t["rho"].sum()) / ref["n_sup"], rel=1e-14)
    assert not tr["grad_depth"][t["clipped"]].any() and tr["grad_depth"][t["quad"]].any()


@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_exact_cases_are_exact(shape):
    """float64 and float32 agree without rounding, and the table's special pixels are there"""
    x = R.exact_case(*shape)
    args = (x["depth"], x["acc"], x["lidar"], x["acc_min"], x["lam"])
    t = R.robust_ops(*args, **R.EXACT)
    for j, k in enumerate(("loss", "mean", "share", "clip_share")):
        assert np.float32(float(t[k])) == x["out4"][j], k
    assert np.abs(t["grad_depth"].numpy() - x["grad_depth"]).max() <= 2 * R.EPS * np.abs(x["grad_depth"]).max()
    if shape[0] * shape[1] > 100:
        assert all(v > 1 for v in x["seen"].values()), x["seen"]
