"""CPU tests of tests/prune_ref.py, the plain-Torch statement of the prune rule and the compaction that the GPU tests
hold csrc/prune.hip to, and its float64 anchor."""
import numpy as np
import torch

import prune_ref as R


def _raw(P, seed):
    gen = torch.Generator().manual_seed(seed)
    scaling = torch.randn((P, 3), generator=gen) * 0.8 - 2.0   # exp: ~40 % of rows have a scale beyond 0.3
    opacity = torch.randn((P, 1), generator=gen) * 2.5 - 2.0   # sigmoid: ~8 % below 1/255
    return scaling, opacity   # float32: both precisions start from the same raw values


def test_rule_bits_boundaries_and_counts():
    lo, hi = R.f32(R.MIN_OPACITY), R.f32(R.MAX_SCALE)
    below, above = np.nextafter(np.float32(lo), np.float32(0)), np.nextafter(np.float32(hi), np.float32(1))
    opac = torch.tensor([0.5, lo, float(below), 0.5, 0.5, 0.5, float("nan"), 0.5], dtype=torch.float32)
    scal = torch.full((8, 3), 0.1, dtype=torch.float32)
    scal[3, 2] = hi              # on the threshold: kept
    scal[4, 1] = float(above)    # one float above: dropped
    scal[5, 0] = float("inf")    # an overflowed exp
    raw_xyz = torch.zeros((8, 3))
    raw_xyz[7, 1] = float("-inf")
    drop = torch.tensor([0, 0, 0, 0, 1, 0, 0, 0], dtype=torch.uint8)
    r = R.reasons_ref(opac, scal, raw=[raw_xyz, opac], drop=drop)
    assert r.tolist() == [0, 0, R.OPACITY, 0, R.SCALE | R.MASK, R.SCALE, R.NONFINITE, R.NONFINITE]
    # a NaN compares false in both tests: without the third bit it survives
    assert R.reasons_ref(opac, scal, raw=[raw_xyz, opac], drop_nonfinite=False).tolist() == \
        [0, 0, R.OPACITY, 0, R.SCALE, R.SCALE, 0, 0]
    assert R.counts_ref(r) == [3, 1, 2, 2, 1]
    rm = R.row_map_ref(r)
    assert rm.dtype == torch.int32 and rm.tolist() == [0, 1, 2, 2, 3, 3, 3, 3, 3]
    t = torch.arange(24.0).reshape(8, 3)
    (out,) = R.compact_ref([t], r)
    assert torch.equal(out, t[[0, 1, 3]])
    for i in (0, 1, 3):   # survivors: row_map is their new row, order kept
        assert torch.equal(out[rm[i]], t[i])


def test_row_map_of_all_none_alternating():
    P = 1001
    for r in (torch.zeros(P, dtype=torch.uint8), torch.ones(P, dtype=torch.uint8),
              (torch.arange(P) % 2).to(torch.uint8)):
        rm = R.row_map_ref(r)
        keep = (r == 0)
        assert int(rm[P]) == int(keep.sum()) == R.counts_ref(r)[0]
        assert torch.equal(rm[:-1][keep].long(), torch.arange(int(keep.sum())))
        assert bool((rm[1:] - rm[:-1] == keep.to(torch.int32)).all())


def test_float32_decisions_match_float64_outside_a_4_ulp_band():
    """The anchor: the float32 rule on float32 activations decides as the float64 rule on float64 activations for every
    row whose float64 activated values all lie more than 4 ulp(f32) away from their threshold; at most 1 % of the rows
    lie inside that band (with these continuous inputs: a handful in 200 000 at most)."""
    P = 200_000
    scaling, opacity = _raw(P, 5)
    s64, o64 = torch.exp(scaling.double()), torch.sigmoid(opacity.double())
    s32, o32 = torch.exp(scaling), torch.sigmoid(opacity)
    r64 = R.reasons_ref(o64, s64)
    r32 = R.reasons_ref(o32, s32)
    lo, hi = R.f32(R.MIN_OPACITY), R.f32(R.MAX_SCALE)
    ulp = lambda x: float(np.spacing(np.float32(x)))  # noqa: E731
    near = ((o64.reshape(P) - lo).abs() <= 4 * ulp(lo)) | ((s64 - hi).abs() <= 4 * ulp(hi)).any(1)
    share = float(near.double().mean())
    assert share <= 0.01, share
    assert torch.equal(r32[~near], r64[~near])
    # the inputs exercise both bits in earnest
    c = R.counts_ref(r64)
    assert 0.02 * P < c[1] < 0.2 * P and 0.02 * P < c[2] < 0.5 * P and c[0] > P // 2


def test_oracle_renders_the_same_without_the_default_dropped_rows():
    """What the GPU test asks of the HIP path, on the CPU oracle first: without the rows the default rule drops, images,
    the survivors' radii and the survivors' gradients are bit-identical (both binning modes of the oracle)."""
    from gs_livm_amd import synthetic as S
    from oracle import oracle as O
    W, H = 160, 96
    O.set_threads(1)   # one fixed summation order for the gradients
    for D in (0, 3):
        sc, keep = R.prune_scene(2000, W, H, 11, D)
        assert 0.03 < 1.0 - keep.mean() < 0.09 and (sc["scales"] > 0.3).any() and (sc["opacities"] < 1 / 255).any()
        dcol, dacc = S.make_upstream_grads(W, H, 11)
        small = R.filter_scene(sc, keep)
        for tight in (False, True):
            a, b = O.forward(sc, tight=tight), O.forward(small, tight=tight)
            for name in ("out_color", "out_depth", "out_acc", "final_T"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (D, tight, name)
            assert np.array_equal(a.radii[keep], b.radii)
            ga, gb = O.backward(a, sc, dcol, dacc), O.backward(b, small, dcol, dacc)
            for name in ga:
                assert np.array_equal(ga[name][keep], gb[name]), (D, tight, name)
                assert not ga[name][~keep].any(), (D, tight, name)   # the dropped rows got no gradient
