"""CPU tests of the contribution reference itself (tests/contrib_ref.py): before the HIP kernel is held to it, the
reference is held to a closed form, to the rendered silhouette, to the oracle's backward (an independent route to the
weight sum) and to the conditions the GPU comparison relies on."""
import functools

import numpy as np
import pytest

import contrib_ref as CR
from helpers import grad_close
from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def _frame(cfg):
    sc = CR.scene(*cfg)
    fr = O.forward(sc)
    return sc, fr, CR.per_gaussian(fr)


def test_one_isotropic_gaussian_equals_the_closed_form_disc():
    fr = O.forward(CR.splat_scene(64, 64, [[31.5, 31.5]], [2.0], 4.0, 0.8))
    A, B, C, o = (float(v) for v in fr.conic_opacity[0])
    assert B == 0.0 and abs(A - C) <= 1e-6 * A and o == np.float32(0.8)  # on the axis: an isotropic conic
    r2_cut = 2.0 * np.log(255.0 * o) / A           # o exp(-r^2 / 2 sigma^2) >= 1/255 with 1 / sigma^2 = A
    ys, xs = np.mgrid[0:64, 0:64]
    r2 = (xs - 31.5) ** 2 + (ys - 31.5) ** 2
    alpha = o * np.exp(-0.5 * A * r2)
    assert np.abs(alpha * 255.0 - 1.0).min() > 1e-3    # no pixel within 1e-3 relative of the cut
    assert fr.fragile.sum() == 0
    r = CR.per_gaussian(fr)
    n = int((r2 <= r2_cut).sum())
    assert 100 < n < 64 * 64 and r["lo"][0] == r["hi"][0] == n
    assert abs(r["wsum64"][0] - alpha[r2 <= r2_cut].sum()) <= 1e-12 * n
    assert abs(r["wmax64"][0] - alpha.max()) <= 1e-15 and r["tiles"][0] >= 4
    assert CR.ellipse_pixels(fr, 0)[:2] == (n, pytest.approx(r["wsum64"][0], rel=1e-13))


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_weight_sums_add_up_to_the_silhouette(cfg):
    _, fr, r = _frame(cfg)
    ok = fr.fragile == 0
    acc = float(fr.out_acc[0][ok].astype(np.float64).sum())
    print("sum wsum64 %.4f  sum out_acc %.4f" % (r["wsum64"].sum(), acc))
    assert abs(r["wsum64"].sum() - acc) <= 1e-6 * acc


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_weight_sum_equals_the_oracle_backward_with_unit_upstream(cfg):
    sc, fr0, _ = _frame(cfg)
    sc = dict(sc)
    P = sc["means3D"].shape[0]
    sc["colors_precomp"] = np.random.default_rng(7).uniform(0, 1, (P, 3)).astype(np.float32)
    sc["shs"] = None
    fr = O.forward(sc)
    assert np.array_equal(fr.n_contrib, fr0.n_contrib)  # (the colours do not bear on the cuts)
    r = CR.per_gaussian(fr)
    dpix = np.zeros((3, fr.H, fr.W), np.float32)
    dpix[0] = (fr.fragile == 0)                         # unit upstream on channel 0, off the fragile pixels
    g = O.backward(fr, sc, dpix, np.zeros((1, fr.H, fr.W), np.float32))
    grad_close(g["dL_dcolors"][:, 0].astype(np.float64), r["wsum64"], "weight_sum")


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_scene_conditions_of_the_gpu_comparison(cfg):
    _, fr, r = _frame(cfg)
    vis = fr.radii > 0
    share = float((fr.fragile != 0).mean())
    sharp = float((r["hi"][vis] == r["lo"][vis]).mean())
    print("fragile share %.2e  unambiguous rows %.4f  rows touching nothing %d" % (share, sharp, int((r["hi"][vis] == 0).sum())))
    assert share < 5e-3 and sharp >= 0.95
    assert (r["hi"][~vis] == 0).all() and (r["wsum64"][~vis] == 0).all() and (r["tiles"][~vis] == 0).all()
    assert (r["wmax64"] <= 0.99).all() and (r["wmax64"] <= r["wsum64"]).all()
    assert (r["wsum64"] <= 0.99 * r["lo"]).all()


def test_float32_yardstick_stays_within_the_recorded_ratio():
    worst_s = worst_m = 0.0
    for cfg in CR.SCENES:
        _, fr, r = _frame(cfg)
        y = CR.yardstick32(fr)
        worst_s = max(worst_s, CR.worst_ratio(y["wsum32"], r["wsum64"]))
        worst_m = max(worst_m, CR.worst_ratio(y["wmax32"], r["wmax64"]))
    print("yardstick32 worst |d| / f64: weight_sum %.3e  weight_max %.3e" % (worst_s, worst_m))
    # CR.YARDSTICK is what the GPU bar is 8 x of: it must be what the reference measures, not a number from elsewhere
    assert 0.5 * CR.YARDSTICK <= max(worst_s, worst_m) <= CR.YARDSTICK


@pytest.mark.parametrize("N,opacity", [(5, 1.0), (6, 0.95), (65, 0.02)])
def test_stack_scenes_behave_as_designed(N, opacity):
    fr = O.forward(CR.stack_scene(N, opacity))
    assert (fr.radii > 0).all() and fr.ranges.shape[0] == 1
    assert np.array_equal(fr.point_list, np.arange(N))  # row order = depth order
    r = CR.per_gaussian(fr)
    K = int(fr.n_contrib.max())
    if opacity == 1.0:     # alpha = 0.99 exactly: T = 0.01 after the first, below 1e-4 after the second
        assert K == 1 and fr.n_contrib.min() == 1
    elif opacity == 0.95:  # T = 0.05^k: the fourth would leave less than 1e-4
        assert K == 3 and fr.fragile.sum() == 0
        assert (r["lo"][:3] == 256).all() and (r["hi"][3:] == 0).all()
    else:
        assert K == N and fr.fragile.sum() == 0 and (r["lo"] == 256).all() and (np.diff(r["wsum64"]) < 0).all()


def test_partly_opaque_stack_stops_its_pixels_at_different_positions():
    fr = O.forward(CR.stack_scene(8, 0.95, sigma_px=6.0))
    r = CR.per_gaussian(fr)
    assert fr.fragile.sum() == 0 and fr.n_contrib.min() == 3 and fr.n_contrib.max() == 8
    assert r["lo"].tolist() == r["hi"].tolist() == [256, 256, 256, 244, 224, 212, 196, 180]
