"""GPU tests: the HIP path against the f64 autograd restatement (tests/ref64.py), not against the f32 oracle.

End to end: the scenes and paths of tests/test_ref64.py, both binning modes, debug and product forwards and backwards,
and a near/far split frame -- images off fragile pixels and all nine gradient groups (helpers.check_against_ref64).
The oracle frame supplies only the discrete structure and the fragile map (ref64.py, module docstring).

At scale: the product forward and backward of 200 003 Gaussians at SH degree 1 and 3 (the compile-time SH variants of
k_preprocess and the SH-staged backward) and of BASELINE C3 near/far; on a fixed sample of visible Gaussians that received a 2-D gradient the HIP's
own 2-D gradients are fed to ref64's per-Gaussian VJP and the 3-D gradient groups compared."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import (GRAD_NAMES, REF64_PATHS, REF64_SCENES, check_against_ref64, grad_close, hip_backward,
                     hip_forward, masked_upstream, ref64_path_scene)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
MODES = ("reference", "culled")


def _hip_vs_f64(sc, seed, dev, near_far_entries=None):
    """Every (mode, debug) combination of one scene against one f64 evaluation; returns the worst ratios."""
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc)
    dcol, dacc = masked_upstream(sc["W"], sc["H"], seed, fr.fragile)
    r = R.render(sc, fr, dcol, dacc, slack=True)
    worst = {}
    runs = [(m, d, False) for m in MODES for d in (True, False)]
    if near_far_entries is not None:
        runs.append(("culled", False, True))
    for mode, debug, near_far in runs:
        if near_far:
            G.set_near_far_hints(near_far_entries, None)
        try:
            t, fwd = hip_forward(sc, dev, debug=debug, ref_rects=(mode == "reference"), near_far=near_far)
            torch.cuda.synchronize()
            if near_far:
                assert G.last_near_far()[0], "the frame was not split"
            got = hip_backward(sc, t, fwd, dcol, dacc, dev, debug=debug)
        finally:
            if near_far:
                G.set_near_far_hints(None, None)
        images = {"out_color": fwd[1].cpu().numpy(), "out_depth": fwd[2].cpu().numpy(),
                  "out_acc": fwd[3].cpu().numpy()}
        w = check_against_ref64(r, fr.fragile, images, {k: got[k] for k in GRAD_NAMES})
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst |d| / bound against f64:", {k: round(v, 3) for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("P,W,H,seed,D", REF64_SCENES)
def test_hip_matches_f64(P, W, H, seed, D, gpu_device):
    sc = S.make_scene(P, W, H, seed, sh_degree=D)
    # the 40 k scene also as a near/far split frame with a small near budget (most tiles go on to the far chain)
    _hip_vs_f64(sc, seed, gpu_device, near_far_entries=8 if P == 40_000 else None)


@pytest.mark.parametrize("kind", REF64_PATHS)
def test_hip_matches_f64_paths(kind, gpu_device):
    sc, seed = ref64_path_scene(kind)
    _hip_vs_f64(sc, seed, gpu_device)


SAMPLE = 4096


@pytest.mark.parametrize("case", ["P200003_D1", "P200003_D3", "C3_near_far"])
def test_per_gaussian_stage_at_scale(case, gpu_device):
    """The product's per-Gaussian backward (k_gaussian_backward with its flag-first skip; at SH degree 3 the SH-staged
    variant) against ref64's per-Gaussian VJP fed with the HIP's own 2-D gradients, on a fixed sample of visible
    Gaussians that received a 2-D gradient; and every one of them has a nonzero 3-D gradient."""
    if case == "C3_near_far":
        P, W, H, seed = S.CONFIGS["C3"]
        sc = S.make_scene(P, W, H, seed)
    else:
        P, W, H, D = 200_003, 320, 200, int(case[-1])
        seed = 31 + D
        sc = S.make_scene(P, W, H, seed, sh_degree=D)
    for k in range(2):  # synchronous, then speculative (a split frame needs the view's history: include/gsraster.h)
        t, fwd = hip_forward(sc, gpu_device, debug=False, near_far=(case == "C3_near_far"))
    torch.cuda.synchronize()
    if case == "C3_near_far":
        assert G.last_near_far()[0], "C3 was not binned near/far"
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device, debug=False)
    # the sample: visible Gaussians that the blend gave a gradient (most of a dense scene's are hidden behind others)
    radii = fwd[4].cpu().numpy()
    two_d = np.concatenate([np.abs(got[k]).reshape(P, -1) for k in
                            ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors")], 1).max(1) > 0
    assert not two_d[radii <= 0].any()
    cand = np.flatnonzero(two_d)
    assert cand.size >= 1000    # (C3: ~3 000 -- its tiles are finished by the nearest splats; all of them are taken)
    idx = np.sort(np.random.default_rng(seed).choice(cand, size=min(SAMPLE, cand.size), replace=False))
    v = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], W, H)
    cl = v["clamped"].cpu().numpy()
    clamped = np.stack([(cl >> k) & 1 for k in range(3)], 1).astype(bool)
    g3 = R.gaussian_vjp(sc, idx, clamped, R.upstream_from_reference_arrays(got, idx))
    ref = {"dL_dmeans3D": g3["means3D"].numpy(), "dL_dcov3D": g3["cov6"].numpy(), "dL_dsh": g3["shs"].numpy(),
           "dL_dscales": g3["scales"].numpy(), "dL_drotations": g3["rotations"].numpy()}
    for k, want in ref.items():
        grad_close(got[k][idx], want, k)
    # k_gaussian_backward skips a Gaussian without a gradient record (flag first): none of these may be skipped
    assert (np.abs(got["dL_dmeans3D"][idx]).max(1) > 0).all()
    conic_nz = np.abs(got["dL_dconic"][idx]).reshape(idx.size, -1).max(1) > 0
    assert (np.abs(got["dL_dscales"][idx]).max(1) > 0)[conic_nz].all()
    assert (np.abs(got["dL_dcov3D"][idx]).max(1) > 0)[conic_nz].all()
