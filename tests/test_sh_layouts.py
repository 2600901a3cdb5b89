"""CPU tests of the SH layouts off the diagonal (tests/sh_layouts.py): the reference side of test_gpu_sh_layouts.py.

The f32 oracle against the f64 restatement on every legal (D, M) pair -- both restate the pair independently
(sh_to_rgb(deg, M, ...) in oracle/gsr_oracle.c, sh_to_rgb(deg, sh, ...) in ref64.py) and run unchanged -- at half of
helpers.check_against_ref64's bars, the headroom the GPU comparison is entitled to; the gradient of the coefficients
beyond the active degree exactly zero on both sides; gradcheck of ref64 on a padded layout; the blind spot of the
diagonal as a fact; and the coverage of the GPU module's cases over the launch cells."""
import numpy as np
import pytest

import ref64 as R
import sh_layouts as L
from helpers import REF64_SCENES, check_against_ref64, masked_upstream
from oracle import oracle as O
from test_ref64 import IMAGES, _gradcheck_and_split_chain_rule, _gradcheck_scene

HEADROOM = 0.5


def _oracle_vs_f64(scene, D, M):
    P, W, H, seed = scene
    sc = L.with_layout(P, W, H, seed, D, M)
    O.set_threads(1)
    fr = O.forward(sc)
    assert (fr.fragile > 0).mean() < 5e-3
    dcol, dacc = masked_upstream(W, H, seed, fr.fragile)
    r = R.render(sc, fr, dcol, dacc, slack=True)
    g = O.backward(fr, sc, dcol, dacc)
    worst = check_against_ref64(r, fr.fragile, {k: getattr(fr, k) for k in IMAGES}, g)
    print("oracle (D, M) = (%d, %d) on %r: worst |d| / bar" % (D, M, scene), {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= HEADROOM, worst
    used = (D + 1) ** 2
    for side, dsh in (("oracle", g["dL_dsh"]), ("ref64", r["dL_dsh"])):   # the unused coefficients: exactly zero
        dsh = np.asarray(dsh).reshape(P, M, 3)
        assert not dsh[:, used:].any(), side
        assert dsh[:, :used].any() or P < 10, side
    return sc, fr, r, (dcol, dacc)


@pytest.mark.parametrize("D,M", L.PAIRS)
def test_oracle_matches_f64_on_every_pair(D, M):
    _oracle_vs_f64(L.SMALL, D, M)


@pytest.mark.parametrize("scene", [L.MID, L.TINY], ids=["P1500", "P7"])
@pytest.mark.parametrize("D,M", L.VARIANT_PAIRS)
def test_oracle_matches_f64_on_the_variant_pairs(D, M, scene):
    _oracle_vs_f64(scene, D, M)


def test_gradcheck_on_a_padded_layout():
    """ref64's gradients are the derivative of ref64's forward at (D, M) = (1, 7) too: three coefficients allocated
    beyond the active degree (the existing check has the diagonal, degree 3, only)."""
    sc = _gradcheck_scene()
    sc["shs"] = np.ascontiguousarray(sc["shs"][:, :7])
    sc["sh_degree"] = 1
    _gradcheck_and_split_chain_rule(sc)


@pytest.mark.parametrize("D,M", [p for p in L.PAIRS if L.natural_degree(p[1]) != p[0]])
def test_degree_read_off_the_coefficient_count_is_refused(D, M):
    """The blind spot of the diagonal: the oracle run at the degree a kernel would read off M, floor(sqrt(M)) - 1, is
    refused by ref64 at D on every pair where the two differ -- so a kernel that derives D from M is outside the bars."""
    P, W, H, seed = L.SMALL
    sc = L.with_layout(P, W, H, seed, D, M)
    O.set_threads(1)
    fr = O.forward(sc)
    dcol, dacc = masked_upstream(W, H, seed, fr.fragile)
    r = R.render(sc, fr, dcol, dacc, slack=True)
    other = dict(sc, sh_degree=L.natural_degree(M))
    fr2 = O.forward(other)
    with pytest.raises(AssertionError):   # the colours
        check_against_ref64(r, fr.fragile, {k: getattr(fr2, k) for k in IMAGES})
    g2 = O.backward(fr2, other, dcol, dacc)
    with pytest.raises(AssertionError):   # and, on their own, the gradients the SH evaluation feeds
        check_against_ref64(r, fr.fragile, None, {k: g2[k] for k in ("dL_dmeans3D", "dL_dsh")})


def test_on_the_diagonal_the_two_degrees_are_the_same_call():
    for P, W, H, seed, D in REF64_SCENES:
        assert L.natural_degree((D + 1) ** 2) == D
    assert all(L.natural_degree((D + 1) ** 2) == D for D in range(4))


def test_launch_cells_restated():
    """Spot checks of the restatement against the launcher's text (csrc/preprocess.hip, launch_preprocess)."""
    c = L.launch_cells(1500, 0, 16, debug=False)
    assert c == dict(forward="rowk12", shs_full=("vec16", "0mod4"), backward="staged", shs_listed=("vec16", "0mod4"),
                     dL_dsh=("vec16", "0mod4"))
    assert L.launch_cells(1536, 1, 4, debug=False)["shs_full"] is None          # whole blocks only: no block-wide copy
    assert L.launch_cells(300, 3, 16, debug=False, shs_ptr=4)["forward"] == "block_copy"     # rows16 == false
    assert L.launch_cells(300, 3, 16, debug=True)["forward"] == "block_copy"                 # the debug copy of cov3D
    assert L.launch_cells(300, 0, 1, debug=False)["forward"] == "plain"
    assert L.launch_cells(300, 0, 1, debug=True)["forward"] == "general"
    assert L.launch_cells(300, 0, 2, debug=False)["shs_full"] == ("scalar", "2mod4")
    assert L.launch_cells(300, 1, 7, debug=False)["dL_dsh"] == ("scalar", "odd")
    assert L.launch_cells(300, 1, 8, debug=False, dsh_ptr=8)["dL_dsh"] == ("scalar", "0mod4")
    assert L.launch_cells(300, 0, 1, debug=False, depth=True)["backward"] == "unstaged+depth"
    assert L.launch_cells(300, 0, 1, debug=False)["shs_listed"] is None


def test_the_gpu_cases_cover_every_cell():
    """All five forward variants, the pipelined ones at every D they admit, staged / unstaged x depth, and both copy
    branches of all three row helpers with 3M = 0 and 2 (mod 4) and odd -- so also with an LDS stride != 3M."""
    reached = set()
    for what, P, D, M, kw in L.gpu_cases():
        reached |= L.cells_reached(L.launch_cells(P, D, M, **kw), D)
    missing = L.required_cells() - reached
    assert not missing, sorted(missing)
    # even 3M (stride 3M + 1) through the scalar branch of every helper, and the two unseen 16-byte row walks
    assert {M for _, _, _, M, kw in L.gpu_cases() if (3 * M) % 4 == 0} >= {4, 8, 12, 16}
