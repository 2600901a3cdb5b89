"""CPU tests: the f64 autograd restatement (tests/ref64.py) checked against finite differences, then the f32 oracle
(oracle/gsr_oracle.c) pinned to it -- images and all nine gradient groups -- on the parity scenes and on one scene per
path and per departure of the reference's backward from the exact derivative (ref64.py, D1-D4)."""
import numpy as np
import pytest
import torch

import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, REF64_PATHS, REF64_SCENES, check_against_ref64, masked_upstream, ref64_path_scene
from oracle import oracle as O

IMAGES = ("out_color", "out_depth", "out_acc")


def _gradcheck_scene():
    """Five splats of a few pixels, opacity <= 0.9, centred well inside 1.3 tanfov, SH degree 3;
    no pixel sits near a cut (checked below)."""
    sc = S.make_scene(5, 40, 36, 3, sh_degree=3)
    rng = np.random.default_rng(7)
    sc["means3D"] = np.array([[-0.3, -0.2, 2.0], [0.25, 0.1, 2.4], [0.0, 0.2, 1.8], [0.2, -0.25, 2.2],
                              [-0.2, 0.25, 2.6]], np.float32)
    sc["scales"] = rng.uniform(0.1, 0.2, (5, 3)).astype(np.float32)
    sc["opacities"] = rng.uniform(0.4, 0.9, (5, 1)).astype(np.float32)
    sc["shs"][:, 0] = rng.uniform(0.5, 1.5, (5, 3)).astype(np.float32)   # no colour near the clamp at 0
    sc["shs"][:, 1:] *= 2.0
    sc["bg"] = np.array([0.3, 0.6, 0.9], np.float32)
    return sc


def _full_graph(sc, fr, params):
    """Images of the whole frame as ONE autograd graph of the 3-D inputs (the cut decisions from these values)."""
    vis = np.flatnonzero(fr.radii > 0)
    leaves = {k: v for k, v in zip(("means3D", "scales", "rotations", "opacities", "shs"), params)}
    _, g = R.per_gaussian(sc, vis, fr.clamped, leaves=leaves)
    bg = torch.from_numpy(sc["bg"].astype(np.float64))
    img = torch.zeros((3, fr.H * fr.W), dtype=torch.float64)
    acc = torch.zeros(fr.H * fr.W, dtype=torch.float64)
    pos = {int(v): i for i, v in enumerate(vis)}
    for tidx in range(fr.ranges.shape[0]):
        ys, xs = R._tile_pixels(fr, tidx)
        pid = torch.as_tensor(ys * fr.W + xs)
        ids = torch.as_tensor([pos[int(i)] for i in fr.point_list[fr.ranges[tidx, 0]:fr.ranges[tidx, 1]]],
                              dtype=torch.long)
        c, _, a, _, _ = R.blend(fr.W, fr.H, R._t(xs), R._t(ys), g["ndc"][ids], g["conic"][ids], g["opacity"][ids],
                                g["color"][ids], g["depth"][ids], bg)
        img = img.index_put((torch.arange(3)[:, None], pid[None]), c.T)
        acc = acc.index_put((pid,), a)
    return torch.cat([img.reshape(-1), acc])


def test_autograd_matches_finite_differences_in_f64():
    """gradcheck of the whole restated forward (per-Gaussian stage + blend, one graph) in f64, away from every cut
    and every departure: ref64's gradients are the derivative of ref64's forward.  Then the split evaluation the other
    tests use (per-tile blend graphs + one per-Gaussian VJP, ref64.render) equals the one-graph gradient."""
    _gradcheck_and_split_chain_rule(_gradcheck_scene())


def _gradcheck_and_split_chain_rule(sc):
    """(also run on a posed camera by tests/test_poses.py)"""
    O.set_threads(1)
    fr = O.forward(sc)
    vis = np.flatnonzero(fr.radii > 0)
    assert vis.size == 5 and (fr.radii[vis] > 4).all() and not fr.clamped.any() and not fr.fragile.any()
    assert not R.beyond_jacobian_clamp(sc, vis).any()
    # no pixel within 1e-3 (relative) of a cut: a finite-difference step cannot flip one
    with torch.no_grad():
        _, g = R.per_gaussian(sc, vis, fr.clamped)
        ys, xs = np.meshgrid(np.arange(fr.H), np.arange(fr.W), indexing="ij")
        mx = ((g["ndc"][:, 0] + 1) * fr.W - 1) * 0.5
        my = ((g["ndc"][:, 1] + 1) * fr.H - 1) * 0.5
        pw = R._power(mx, my, g["conic"], R._t(xs.ravel()), R._t(ys.ravel()))
        alpha = g["opacity"] * torch.exp(pw)
        assert (alpha < 0.9).all() and float((alpha * 255.0).log().abs().min()) > 1e-3
        assert float(torch.cumprod(1 - torch.where(alpha >= 1 / 255, alpha, 0 * alpha), 1).min()) > 2e-4
    params = tuple(torch.from_numpy(sc[k][vis].astype(np.float64)).requires_grad_(True)
                   for k in ("means3D", "scales", "rotations", "opacities", "shs"))
    assert torch.autograd.gradcheck(lambda *p: _full_graph(sc, fr, p), params, eps=1e-6, atol=1e-7, rtol=1e-4)
    # the split chain rule of ref64.render against the one graph
    rng = np.random.default_rng(3)
    dcol = rng.standard_normal((3, fr.H, fr.W))
    dacc = rng.standard_normal((1, fr.H, fr.W))
    out = _full_graph(sc, fr, params)
    up = torch.from_numpy(np.concatenate([dcol.reshape(-1), dacc.reshape(-1)]))
    full = torch.autograd.grad(out, params, up)
    r = R.render(sc, fr, dcol, dacc)
    for k, gf in zip(("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dsh"), full):
        np.testing.assert_allclose(r[k][vis].reshape(gf.shape), gf.numpy(), rtol=1e-10, atol=1e-14 * float(gf.abs().max()))


def _oracle_vs_f64(sc, seed):
    O.set_threads(1)
    fr = O.forward(sc)
    assert (fr.fragile > 0).mean() < 5e-3
    dcol, dacc = masked_upstream(sc["W"], sc["H"], seed, fr.fragile)
    r = R.render(sc, fr, dcol, dacc, slack=True)
    g = O.backward(fr, sc, dcol, dacc)
    images = {k: getattr(fr, k) for k in IMAGES}
    check_against_ref64(r, fr.fragile, images, g)
    ok = fr.fragile == 0
    assert np.array_equal(r["n_contrib"][ok], fr.n_contrib[ok])
    return fr, r, g


@pytest.mark.parametrize("P,W,H,seed,D", REF64_SCENES)
def test_oracle_matches_f64(P, W, H, seed, D):
    _oracle_vs_f64(S.make_scene(P, W, H, seed, sh_degree=D), seed)


@pytest.mark.parametrize("kind", REF64_PATHS)
def test_oracle_matches_f64_paths(kind):
    sc, seed = ref64_path_scene(kind)
    fr, r, g = _oracle_vs_f64(sc, seed)
    vis = fr.radii > 0
    if kind == "colors_precomp":
        assert g["dL_dsh"].size == 0 and np.abs(r["dL_dcolors"]).max() > 0
    elif kind == "cov3D_precomp":
        assert np.abs(r["dL_dcov3D"]).max() > 0 and not g["dL_dscales"].any()
    elif kind == "opaque":
        assert (fr.conic_opacity[vis, 3] >= 0.99).sum() >= 100
    elif kind == "jacobian_clamp":
        out = np.zeros(fr.P, bool)
        out[vis] = R.beyond_jacobian_clamp(sc, np.flatnonzero(vis)).numpy()
        assert out.sum() >= 10 and (np.abs(r["dL_dconic"][out]).max(axis=(1, 2)) > 0).sum() >= 10
    elif kind == "sh_clamp":
        cl = fr.clamped.astype(bool) & vis[:, None]
        assert cl.sum() >= 100 and not r["dL_dsh"].transpose(0, 2, 1)[cl].any()


@pytest.mark.parametrize("kind,departure", [("opaque", "D1"), ("jacobian_clamp", "D3"), ("scale_modifier", "D4")])
def test_each_departure_is_needed(kind, departure):
    """Each departure modelled in ref64.py is real: without it the exact derivative disagrees with the oracle (the
    reference's definition) beyond the bound on the scene that exercises it.  (D2, the 1e-7 in denom2inv, moves no
    gradient here by more than 1e-5 of its row and is modelled but below any bar.)"""
    sc, seed = ref64_path_scene(kind)
    O.set_threads(1)
    fr = O.forward(sc)
    dcol, dacc = masked_upstream(sc["W"], sc["H"], seed, fr.fragile)
    g = O.backward(fr, sc, dcol, dacc)
    exact = R.render(sc, fr, dcol, dacc, departures=False, slack=True)
    failed = []
    for k in GRAD_NAMES:
        try:
            check_against_ref64(exact, fr.fragile, None, {k: g[k]})
        except AssertionError:
            failed.append(k)
    assert failed, departure
