"""CPU tests of the sweep-admission reference (tests/seed_ref.py): the conditions the GPU tests of
tests/test_gpu_seed.py rely on, asserted without a device."""
import numpy as np
import pytest
import torch

import seed_ref as SR


def _as_got(y):
    return {k: y[k] for k in ("codes", "counts", "index", "pixel", "z", "covs", "rgb")}


@pytest.mark.parametrize("case", SR.CASE_NAMES + SR.EXACT_NAMES)
def test_ops_in_float64_equal_the_loop(case):
    x = SR.inputs(case)
    t, y = SR.reference(case)["truth"], SR.admit_ops(x, torch.float64)
    for k in ("codes", "counts", "index", "pixel", "z", "xyz", "covs", "rgb"):
        if t[k] is None:
            assert y[k] is None, k
        else:
            assert np.array_equal(SR._np(y[k]), np.asarray(t[k])), (case, k)


@pytest.mark.parametrize("case", SR.CASE_NAMES)
def test_every_code_is_populated_and_few_points_are_fragile(case):
    x, ref = SR.inputs(case), SR.reference(case)
    t = ref["truth"]
    assert x["n"] <= 6000 and (x["W"], x["H"]) in ((70, 50), (33, 17))
    assert int(t["counts"].sum()) == x["n"]
    possible = SR.possible_codes(x)
    for code in range(6):
        share = t["counts"][code] / x["n"]
        if code in possible:
            assert share >= SR.MIN_SHARE, (case, code, share)
        else:
            assert t["counts"][code] == 0, (case, code)
    assert ref["n_fragile"] <= 0.01 * x["n"], (case, ref["n_fragile"])
    print(case, "shares", np.round(t["counts"] / x["n"], 3), "fragile", ref["n_fragile"])


def test_the_cases_cover_what_they_claim():
    xs = {c: SR.inputs(c) for c in SR.CASE_NAMES}
    assert len(SR.possible_codes(xs["full_70x50"])) == 6 == len(SR.possible_codes(xs["tiny_33x17"]))
    for k in SR.OPTIONAL:               # each optional input present and absent
        assert any(x[k] is None for x in xs.values()) and any(x[k] is not None for x in xs.values()), k
    assert {x["one_per_pixel"] for x in xs.values()} == {True, False}
    assert {x["radius"] for x in xs.values()} == {0, 1, 2, 3}
    for x in xs.values():
        assert x["K"][0, 0] != x["K"][1, 1]
    R = xs["posed_70x50"]["T_cw"][:, :3]
    assert (np.abs(R) > 1e-3).all()     # a posed camera: a transposed R is another matrix


@pytest.mark.parametrize("case", SR.CASE_NAMES)
def test_the_float32_restatement_sits_inside_the_bars(case):
    x, ref = SR.inputs(case), SR.reference(case)
    r = SR.ratios(_as_got(ref["f32"]), ref, x)
    print(case, r)
    assert r["codes"] == 0 and r["rows"] and r["counts"] <= 1.0
    for k in ("z", "var", "rgb"):
        assert r.get(k, 0.0) <= 1.0, (case, k, r[k])


@pytest.mark.parametrize("case", SR.CASE_NAMES)
def test_a_permuted_sweep_admits_the_same_points(case):
    x = SR.inputs(case)
    t = SR.reference(case)["truth"]
    # by construction no two survivors of one pixel have the same z, in float64 or rounded to float32 (the tie is
    # the one place where the order of the input decides)
    surv = np.nonzero((t["codes"] == SR.ADMITTED) | (t["codes"] == SR.DUPLICATE))[0]
    pix = t["iy"][surv] * x["W"] + t["ix"][surv]
    for z in (t["proj"]["z"][surv], t["proj"]["z"][surv].astype(np.float32)):
        assert len({(int(p), float(v)) for p, v in zip(pix, z)}) == len(surv)
    perm = np.random.default_rng(5).permutation(x["n"])
    xp = dict(x, points=x["points"][perm], covs=None if x["covs"] is None else x["covs"][perm])
    tp = SR.admit64(xp)
    assert np.array_equal(np.sort(perm[tp["index"]]), t["index"])
    assert np.array_equal(tp["codes"], t["codes"][perm])


def test_exact_cases_carry_their_special_points():
    x, t = SR.inputs("exact_17x33"), SR.reference("exact_17x33")["truth"]
    k = len(SR.EXACT_SPECIAL_CODES)
    assert tuple(int(c) for c in t["codes"][-k:]) == SR.EXACT_SPECIAL_CODES
    assert (t["counts"] > 0).all()                       # every code occurs
    pts = x["points"]
    assert pts[-7].tobytes() == pts[-6].tobytes()        # the identical pair: the lower index wins
    assert t["pixel"][list(t["index"]).index(x["n"] - k + 3)] == (x["H"] - 1) * x["W"]      # X == -0.5: pixel 0 of the row
    t0 = SR.reference("exact_n0")["truth"]
    assert t0["counts"].sum() == 0 and t0["index"].shape == (0,)


def test_end_to_end_scene_with_the_oracle():
    """The three conditions of the end-to-end GPU test, on the oracle's frames: the admitted points lie in the hole,
    appending them closes it, and a second admission of the same sweep admits next to nothing."""
    from oracle import oracle as O
    s = SR.hole_scene()
    H, W = s["H"], s["W"]
    assert s["xyz"].shape[0] <= 600 and (W, H) == (70, 50)

    def admit(xyz, scales, rgbs):
        fr = O.forward(SR.oracle_scene(xyz, scales, rgbs), keep_handle=False)
        x = dict(points=s["sweep"], T_cw=s["T_cw"], K=s["K"], H=H, W=W, min_depth=0.2, max_depth=float("inf"),
                 depth=fr.out_depth[0], acc=fr.out_acc[0], lidar=None, image=np.clip(fr.out_color, 0, 1), covs=None,
                 exposure=None, radius=1, one_per_pixel=True, **SR.E2E)
        return SR.admit64(x), fr

    a1, fr1 = admit(s["xyz"], s["scales"], s["rgbs"])
    m1 = len(a1["index"])
    inside = SR.in_hole(a1["pixel"], W)
    print("admitted", m1, "in the hole", inside.mean())
    assert m1 >= 200 and inside.mean() >= 0.9
    sig = np.sqrt(a1["covs"][:, [0, 4, 8]])
    xyz2, sc2 = np.concatenate([s["xyz"], a1["xyz"]]), np.concatenate([s["scales"], sig.astype(np.float32)])
    a2, fr2 = admit(xyz2, sc2, np.concatenate([s["rgbs"], a1["rgb"].astype(np.float32)]))
    hit = np.zeros(H * W, bool)
    hit[(a1["iy"] * W + a1["ix"])[a1["ix"] >= 0]] = True
    sel = hit & SR.in_hole(np.arange(H * W), W)
    closed = (fr2.out_acc.reshape(-1)[sel] >= SR.E2E["acc_min"]).mean()
    print("hole pixels closed", closed, "second admission", len(a2["index"]), "of", m1)
    assert (fr1.out_acc.reshape(-1)[sel] < SR.E2E["acc_min"]).mean() >= 0.5     # it was a hole
    assert closed >= 0.9
    assert len(a2["index"]) <= 0.1 * m1
