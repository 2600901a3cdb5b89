"""CPU tests of the oracle on the scenes of tests/nonfinite.py: every cull boundary against the outcome written out from
the reference's source line, and the poisoned scenes' containment properties -- what a non-finite row may and may not
touch.  tests/test_gpu_nonfinite.py holds the HIP path to the same frames."""
import numpy as np
import pytest

import nonfinite as NF
from gs_livm_amd import synthetic as S
from oracle import oracle as O

MODES = (False, True)   # the oracle's `tight`: the reference's rectangles, the product's culled ones


def _frames(sc):
    O.set_threads(1)
    return [O.forward(sc, tight=t) for t in MODES]


@pytest.mark.parametrize("name", sorted(NF.BOUNDARIES))
def test_boundary_rows_fall_on_the_references_side(name):
    sc, ex = NF.BOUNDARIES[name]()
    for fr in _frames(sc):
        vis = np.array(ex["visible"])
        assert np.array_equal(fr.radii > 0, vis), (name, fr.radii)
        assert not fr.tiles_touched[~vis].any()
    ref, tight = _frames(sc)
    assert (ref.tiles_touched[vis] > 0).all()
    if name != "alpha_out":   # (an opacity below 1/255 has no footprint: the culled mode emits nothing for it)
        assert (tight.tiles_touched[vis] > 0).all()


def test_the_scale_modifier_pair_straddles_the_limit():
    a, b = NF.scale_modifier_pair(0.7)
    assert b == NF.up(a) and np.float32(0.7) * a <= np.float32(0.3) < np.float32(0.7) * b
    # and the raw scales themselves are far from 0.3f: the decision is the PRODUCT's
    assert a > np.float32(0.42)


@pytest.mark.parametrize("which", [0, 1])
def test_alpha_cut_at_exactly_one_255th(which):
    """alpha == 1/255 blends, the float below it does not -- in the forward (pixel, n_contrib), in the preprocess cull
    and footprint box (the culled mode still hands the centre pixel's tile the row) and in the backward."""
    sc, ex = NF.alpha_cut(which)
    dcol, dacc = NF.centre_upstream()
    for tight, fr in zip(MODES, _frames(sc)):
        px = fr.out_color[:, NF.CY, NF.CX]
        g = O.backward(fr, sc, dcol, dacc)
        if ex["contributes"]:
            assert fr.n_contrib[NF.CY, NF.CX] == 1 and fr.tiles_touched[0] > 0
            assert np.abs(px - ex["centre"]).max() <= 1e-4 and not np.array_equal(px, NF.BG)
            assert g["dL_dopacity"][0, 0] != 0
            tile = (NF.CY // 16) * ((NF.W0 + 15) // 16) + NF.CX // 16
            assert tile in (fr.keys >> np.uint64(32)).tolist()
        else:
            assert fr.n_contrib[NF.CY, NF.CX] == 0 and np.array_equal(px, NF.BG)
            assert np.array_equal(fr.out_color, np.broadcast_to(NF.BG[:, None, None], fr.out_color.shape))
            assert g["dL_dopacity"][0, 0] == 0 and not any(v.any() for v in g.values())
            assert fr.tiles_touched[0] == (0 if tight else 2)


def test_alpha_clamp_leaves_one_minus_099f():
    sc, ex = NF.alpha_clamp()
    for fr in _frames(sc):
        assert fr.final_T[NF.CY, NF.CX] == ex["final_T"] and fr.n_contrib[NF.CY, NF.CX] == 1


def test_indefinite_covariance_is_kept_and_skipped_where_power_is_positive():
    sc, _ = NF.indefinite_cov()
    ref, tight = _frames(sc)
    co = ref.conic_opacity[0]
    assert co[0] < 0 < co[2] and co[0] * co[2] - co[1] * co[1] < 0          # det < 0: kept by `det == 0`
    assert np.array_equal(ref.tiles_touched, tight.tiles_touched)            # indefinite conic: no culling
    # along the centre row the row-0 splat has power > 0 and is skipped, along the centre column it blends
    sc1 = dict(sc, means3D=sc["means3D"][1:], opacities=sc["opacities"][1:], shs=sc["shs"][1:],
               cov3D_precomp=sc["cov3D_precomp"][1:])
    alone = O.forward(sc1)
    x = NF.CX + 2
    assert np.array_equal(ref.out_color[:, NF.CY, x], alone.out_color[:, NF.CY, x])
    assert not np.array_equal(ref.out_color[:, NF.CY + 1, NF.CX], alone.out_color[:, NF.CY + 1, NF.CX])
    for k in ("out_color", "out_depth", "out_acc", "final_T"):
        assert np.array_equal(getattr(ref, k), getattr(tight, k)), k


def test_det_zero_row_really_has_det_zero():
    """The row is in the table only because its det IS 0.0f: cxx + 0.3f == 0 and cxy == 0 exactly."""
    sc, _ = NF.det_zero()
    f = np.float32
    fx = f(NF.W0) / (f(2.0) * f(sc["tanfovx"]))
    assert fx == 16 and f(NF.H0) / (f(2.0) * f(sc["tanfovy"])) == 16
    cxx = (fx / f(16.0)) * (fx / f(16.0)) * sc["cov3D_precomp"][:, 0]
    assert cxx[0] + f(0.3) == 0 and cxx[1] + f(0.3) > 0
    ref, _ = _frames(sc)
    co = ref.conic_opacity[1]
    assert np.isfinite(co).all() and co[2] * co[0] > 0                       # the neighbour: tiny positive det, kept


# ---- poisoned scenes ---------------------------------------------------------------------------------------------
def _poison_cases():
    out = []
    for D in (0, 3):
        out += [(D,) + c for c in NF.cases(D)] + [(D, "everything", "", ())]
    return out


def _scene(D, field, value, rows):
    return NF.everything(D) if field == "everything" else NF.poisoned(D, field, value, rows)


def _ids(c):
    return "D%d-%s-%s-%s" % (c[0], c[1], c[2], "all" if len(c[3]) > 1 else "".join(map(str, c[3])))


@pytest.mark.parametrize("case", _poison_cases(), ids=_ids)
def test_poison_stays_in_its_rows_and_its_tiles(case):
    sc, clean, rows = _scene(*case)
    base = O.forward(clean, keep_handle=False)
    frames = _frames(sc)
    for k in ("radii", "out_color", "out_depth", "out_acc", "final_T", "fragile"):  # the binning modes agree
        assert NF.same(getattr(frames[0], k), getattr(frames[1], k)), k
    for fr in frames:
        assert (fr.fragile > 0).mean() < 5e-3                    # the bar of check_forward, held by the oracle alone
        # conversions are defined: no radius is INT_MIN, no rectangle is the whole grid, the lists add up
        assert (fr.radii >= 0).all() and fr.R == int(fr.tiles_touched.sum())
        assert (fr.tiles_touched[list(rows)] <= 1).all()     # (every poisoned row sits on one tile of its own)
        # outside the tiles a poisoned row reaches -- in this frame or, unpoisoned, in the clean one -- nothing moves
        far = ~(NF.reached_pixels(fr, rows) | NF.reached_pixels(base, rows))
        assert far.any()
        for k in ("out_color", "out_depth", "out_acc", "final_T"):
            assert np.array_equal(getattr(fr, k)[..., far], getattr(base, k)[..., far]), k
        # gradients: a non-finite row is a poisoned row.  One exception, the reference's own arithmetic: a row with a
        # non-finite COLOUR (precomputed, or from an SH coefficient of +-Inf; a NaN sum is clamped to 0) puts it into
        # accum_rec of every splat in front of it on the same pixel (backward.cu:527-533), so rows sharing a tile with
        # it may turn NaN too -- and only those.
        dcol, dacc = S.make_upstream_grads(NF.PW, NF.PH, NF.SEED)
        keep = (fr.fragile == 0).astype(np.float32)
        with np.errstate(all="ignore"):
            g = O.backward(fr, sc, dcol * keep, dacc * keep)
        bad = set()
        for v in g.values():
            if v.size:
                bad |= set(np.flatnonzero(~np.isfinite(v.reshape(NF.PP, -1)).all(1)).tolist())
        allowed = set(rows)
        if not np.isfinite(fr.out_color).all():
            tiles = (fr.keys >> np.uint64(32))
            shared = np.isin(tiles, tiles[np.isin(fr.point_list, np.asarray(rows, np.uint32))])
            allowed |= set(fr.point_list[shared].tolist())
        else:
            assert np.isfinite(fr.out_depth).all() and np.isfinite(fr.out_acc).all()
        assert bad <= allowed, sorted(bad - allowed)
        assert len(bad) < NF.PP // 4


def test_nan_radius_rows_keep_one_tile_and_radius_zero():
    """A NaN scale or rotation: my_radius is NaN, the conversion gives 0 (cvt.rzi / v_cvt_i32_f32), the rectangle of
    radius 0 is the one tile under the mean, the conic is NaN (power NaN passes `power > 0`), alpha = min(0.99, NaN):
    the row paints its tile at 0.99 and reports radii == 0."""
    for field in ("scale", "rotation"):
        sc, clean, rows = NF.poisoned(0, field, "nan", NF.POISON_ROWS)
        for fr in _frames(sc):
            assert not fr.radii[list(rows)].any() and (fr.tiles_touched[list(rows)] == 1).all()
            for r in rows:
                tx, ty = NF.ROW_TILES[r]
                inst = np.flatnonzero(fr.point_list == r)
                assert len(inst) == 1 and int(fr.keys[inst[0]] >> np.uint64(32)) == ty * 5 + tx
                # the row's own tile: every pixel has taken alpha 0.99 from it -- T_final <= 0.01 T_before
                assert (fr.final_T[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] <= np.float32(0.0100001)).all()


@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
def test_a_nonfinite_opacity_paints_and_both_modes_agree(value):
    """NaN and +Inf paint the whole rectangle at 0.99; -Inf paints where exp(power) has underflowed (-Inf * 0 = NaN) and
    nowhere else.  Deleting the row is NOT the same frame -- in either binning mode."""
    sc, clean, rows = NF.poisoned(0, "opacity", value, (NF.DIAGONAL_ROW,))
    gone = {k: (np.delete(v, rows, 0) if isinstance(v, np.ndarray) and v.shape[:1] == (NF.PP,) else v)
            for k, v in sc.items()}
    without = O.forward(gone, keep_handle=False)
    for fr in _frames(sc):
        moved = (fr.out_color != without.out_color).any(0)
        tx, ty = NF.ROW_TILES[NF.DIAGONAL_ROW]
        assert moved.any() and not moved[NF.reached_pixels(fr, rows) == 0].any()
        assert float(np.abs(fr.out_color - without.out_color).max()) > 0.1
        if value != "-inf":
            assert moved[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].mean() > 0.9
        else:
            assert 0 < moved.sum() < 64


def test_mark_visible_with_nonfinite_means():
    """present = !(z_view <= 0.2): a NaN depth is `visible` (the comparison is false), +Inf is, -Inf is not."""
    sc = NF.base(0)
    m = sc["means3D"][:8].copy()
    m[0, 2], m[1, 2], m[2, 2], m[3, 0], m[4, 1], m[5, 2], m[6, 2] = (np.nan, np.inf, -np.inf, np.nan, np.inf,
                                                                     np.float32(0.2), NF.up(0.2))
    got = O.mark_visible(m, sc["viewmatrix"])
    # rows 3 and 4: 0 * NaN and 0 * Inf in the dot product with the view matrix's third column are NaN
    assert got.tolist() == [True, True, False, True, True, False, True, bool(m[7, 2] > 0.2)]
