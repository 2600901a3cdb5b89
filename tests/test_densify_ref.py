"""CPU anchor of tests/densify_ref.py, the restatement csrc/densify.hip is held to (test_gpu_densify.py): Philox known
answers, the normal stream, the float32 restatement inside every bar on every input of the GPU tests, the mark rule's
wording on the rows that decide it, and the in-place layout against upstream's densify_and_clone + densify_and_split
written in Torch ops."""
import numpy as np
import pytest
import torch

import densify_cases as Cs
import densify_ref as D


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = D.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert " ".join("%08x" % x for x in got) == want
    batch = D.philox4x32_10(np.array([k[0] for k in kat], dtype=np.uint32)[:1].repeat(3, 0), kat[0][1])
    assert (batch == batch[0]).all()                       # vectorised over counters


def test_uniforms_are_exact_and_strictly_inside_the_unit_interval():
    o = np.array([0, 1, 511, 512, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    u = D.uniforms(o)                                      # (asserts exactness against float64 itself)
    assert u.dtype == np.float32 and u.min() == np.float32(2.0 ** -24) and u.max() < 1.0
    assert np.sqrt(-2.0 * np.log(float(u.min()))) <= D.R_MAX * (1 + 1e-12)
    # the constant of the split: ln 1.6 to within half a float32 ulp
    assert abs(float(D.LN_1_6) - np.log(1.6)) <= 2.0 ** -25 * 0.5


def test_the_normal_stream_is_standard_normal():
    n = 200_000
    z = np.concatenate([D.normals(12345, np.arange(n // 6), c, np.float32)[0] for c in (0, 1)]).reshape(-1)
    z = z[:n].astype(np.float64)
    se_mean, se_var = 1.0 / np.sqrt(n), np.sqrt(2.0 / n)
    print("normal stream: mean %.2e  variance %.4f" % (z.mean(), z.var()))
    assert abs(z.mean()) <= 4 * se_mean and abs(z.var() - 1.0) <= 4 * se_var
    # the three components are uncorrelated, and the two children of a row differ
    z0, z1 = (D.normals(7, np.arange(20_000), c, np.float64)[0] for c in (0, 1))
    assert np.abs(np.corrcoef(z0.T) - np.eye(3)).max() <= 4 / np.sqrt(20_000)
    assert not np.isclose(z0, z1).all(1).any()
    # (seed, row, child) decide a sample: not the batch it is drawn in
    assert np.array_equal(D.normals(7, [5, 19_999], 1, np.float32)[0], D.normals(7, np.arange(20_000), 1, np.float32)[0][[5, 19_999]])


@pytest.mark.parametrize("P", Cs.ACC_SIZES)
def test_float32_accumulate_is_inside_its_bar(P):
    views, stats0, touched = Cs.accumulate_case(P)
    s32, s64 = stats0.copy(), np.where(touched[:, None], np.zeros((P, 3)), np.nan)
    for radii, g in views:
        s32, s64 = D.accumulate(s32, radii, g, np.float32), D.accumulate(s64, radii, g, np.float64)
    assert np.array_equal(s32.view(np.uint32)[~touched], stats0.view(np.uint32)[~touched])
    t = touched
    assert np.array_equal(s32[t, 1:], s64[t, 1:]) and (s32[t, 1] >= 1).all()
    # in float32 itself the only rounding that the bar's K does not count is the products' fall into the subnormals
    err = np.abs(s32[t, 0].astype(np.float64) - s64[t, 0])
    small = s64[t, 0] < 1e-15
    assert (err[~small] <= D.K_SUM * D.ULP * s64[t, 0][~small]).all()
    assert (err[small] <= 1e-18).all()
    if P >= 255:                                           # every kind of row occurs
        for radii, g in views:
            n = np.sqrt(g[:, 0].astype(np.float64) ** 2 + g[:, 1].astype(np.float64) ** 2)
            assert (radii == 0).any() and (radii < 0).any() and (radii > 0).any()
            assert np.isnan(n).any() and np.isinf(n).any() and (n == 0).any() and (n > 1e7).any() and (n < 1e-15).any()


def test_mark_rule_on_the_rows_that_decide_it():
    stats, scaling, want = Cs.mark_boundary_case()
    s = scaling[np.isfinite(scaling).all(1)].max(1)
    assert ((s == 0) | (np.abs(np.exp(s.astype(np.float64)) - 1.0) > 1e-5)).all()   # exp(0) = 1 exactly; the rest is far
    kinds, offsets, counts = D.mark(stats, scaling, Cs.GRAD_THRESHOLD, 1.0)
    assert kinds.tolist() == want.tolist()
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(want != 0)]).tolist()
    assert counts == [int((want != 0).sum()), int((want == 1).sum()), int((want == 2).sum())]


@pytest.mark.parametrize("P", Cs.MARK_SIZES[:-1])
def test_mark_cap_and_margins(P):
    for pattern in Cs.MARK_PATTERNS:
        stats, scaling, cand = Cs.mark_case(P, pattern)
        assert D.size_margin(scaling, Cs.SIZE_THRESHOLD) > 1e-5, (P, pattern)
        kinds, offsets, counts = D.mark(stats, scaling, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD)
        assert np.array_equal(kinds != 0, cand) and counts[0] == int(cand.sum()) == counts[1] + counts[2]
        total = counts[0]
        for max_new in (-1, 0, 1, total - 1, total, total + 1):
            if max_new < -1:
                continue
            k, o, c = D.mark(stats, scaling, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD, max_new)
            n = total if max_new < 0 else min(total, max_new)
            first = np.nonzero(cand)[0][:n]                # the first max_new candidates in row order win
            assert np.array_equal(np.nonzero(k)[0], first) and np.array_equal(k[first], kinds[first])
            assert c[0] == n == int(o[-1]) and c[1] + c[2] == n and (np.diff(o) == (k != 0)).all()


def test_big_mark_case_keeps_its_margin():
    for pattern in ("0.05", "one_per_workgroup"):
        stats, scaling, cand = Cs.mark_case(Cs.MARK_SIZES[-1], pattern)
        assert D.size_margin(scaling, Cs.SIZE_THRESHOLD) > 1e-5
        assert (len(stats) + 255) // 256 > 1024 and cand[1024 * 256:].any()


def _upstream(leaves, kinds, z0, z1):
    """densify_and_clone, then densify_and_split with N = 2, as upstream lays the rows out: clones appended, the two
    children of every split row appended, the split parents removed -- Torch ops in float64, fed the same normals"""
    t = [torch.from_numpy(a.astype(np.float64)) for a in leaves]
    kinds = torch.from_numpy(kinds.astype(np.int64))
    clone, split = kinds == 1, kinds == 2
    grown = [torch.cat([a, a[clone]], 0) for a in t]                              # densify_and_clone
    xyz, fdc, frest, scaling, rot, opac = t
    stds = torch.exp(scaling[split]).repeat(2, 1)
    samples = torch.cat([torch.from_numpy(z0), torch.from_numpy(z1)], 0)          # torch.normal(mean = 0, std = stds) / stds
    q = torch.nn.functional.normalize(rot[split]).repeat(2, 1)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)   # build_rotation
    new_xyz = torch.bmm(R, (stds * samples).unsqueeze(-1)).squeeze(-1) + xyz[split].repeat(2, 1)
    new_scaling = torch.log(torch.exp(scaling[split]).repeat(2, 1) / (0.8 * 2))
    rep = lambda a: a[split].repeat(2, *([1] * (a.dim() - 1)))  # noqa: E731
    new = [new_xyz, rep(fdc), rep(frest), new_scaling, rep(rot), rep(opac)]
    grown = [torch.cat([a, b], 0) for a, b in zip(grown, new)]                    # densification_postfix
    keep = torch.cat([~split, torch.ones(int(clone.sum()) + 2 * int(split.sum()), dtype=torch.bool)])
    return [a[keep].numpy() for a in grown]                                       # prune_points(prune_filter)


def _sorted_rows(leaves):
    m = np.concatenate([a.reshape(a.shape[0], -1).astype(np.float64) for a in leaves], 1)
    return m[np.lexsort(m.T[::-1])]


@pytest.mark.parametrize("P,M", Cs.APPLY_CASES)
def test_in_place_layout_is_upstreams_multiset_and_float32_is_inside_the_bars(P, M):
    leaves, moments, stats, kinds, offsets = Cs.apply_case(P, M)
    assert (kinds == 1).any() or P == 1
    assert (kinds == 2).any()
    seed = 0xC0FFEE1234567
    out64, mom, st = D.apply(leaves, kinds, offsets, seed, np.float64, moments, stats)
    out32, _, _ = D.apply(leaves, kinds, offsets, seed, np.float32)
    n_new = int(offsets[-1])
    assert all(a.shape[0] == P + n_new for a in out64)
    sp = np.nonzero(kinds == 2)[0]
    z0, z1 = (D.normals(seed, sp, c, np.float64)[0] for c in (0, 1))
    up = _upstream(leaves, kinds, z0, z1)
    assert up[0].shape[0] == P + n_new
    # the same multiset of rows; log(exp(s) / 1.6) against s - fl32(ln 1.6) differ by the constant's rounding (< 3e-8)
    a, b = _sorted_rows(out64), _sorted_rows(up)
    assert np.allclose(a, b, rtol=0, atol=1e-7 + 1e-12 * np.abs(b).max())
    # float32 alone inside the bars of the split rows; everything else is copied bit for bit
    c64 = D.split_children(leaves[0], leaves[3], leaves[4], sp, seed, np.float64)
    dst = P + offsets[sp]
    zero = np.zeros((sp.size, 3))
    for rows, truth in ((sp, c64[0]), (dst, c64[1])):
        assert (np.abs(out32[0][rows] - truth) <= D.xyz_bar(zero, c64[3], leaves[0][sp])).all()
        assert (np.abs(out32[3][rows] - c64[2]) <= D.scale_bar(zero, leaves[3][sp])).all()
    for k in (1, 2, 4, 5):
        assert np.array_equal(out32[k], out64[k])
    none = np.nonzero(kinds == 0)[0]
    for k in range(6):
        assert np.array_equal(out64[k][none], leaves[k][none].astype(np.float64))
    cl = np.nonzero(kinds == 1)[0]
    for a, b in zip(mom, moments):                          # clone parents keep their moments; new rows and split parents: zero
        assert np.array_equal(a[cl], b[cl]) and not a[P:].any() and not a[sp].any()
    assert np.array_equal(st[cl], stats[cl]) and not st[P:].any() and not st[sp].any()
