"""GPU tests of the per-Gaussian blend contribution (csrc/render.hip k_contribution_tile, csrc/contrib.hip, through
gsr_contribution / gsr_contribution_finish, gs_livm_amd.contribution, GrowableGaussians' contribution statistics).

Reference: tests/contrib_ref.py on the CPU oracle's frames (held to a closed form, to the silhouette and to the oracle's
backward by tests/test_contrib_ref.py).  Counts are exact off the oracle's fragile pixels; weights are held to
    |weight_sum - wsum64| <= B wsum64 + 2^-33 tiles + 0.99 (hi - lo)
with B = 8 x the float32 yardstick's worst ratio (contrib_ref.B = 6.16e-6), 2^-33 per tile the rounding of the fixed-point
accumulation and 0.99 the most one ambiguous pixel can add; weight_max likewise without the tiles term."""
import functools

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi
from gs_livm_amd import synthetic as S

import contrib_ref as CR
from helpers import grad_close, hip_backward, hip_forward
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(cfg):
    sc = CR.scene(*cfg)
    fr = O.forward(sc)
    return sc, fr, CR.per_gaussian(fr)


def _run(sc, dev, min_pixels=1, min_weight=0.0, **fwd_kw):
    """(fwd, numpy dict) of one forward + contribution, the outputs prefilled with 0xFF bytes"""
    _, fwd = hip_forward(sc, dev, debug=False, **fwd_kw)
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    ff = lambda dt, *shape: torch.full(shape, 0xFF, dtype=torch.uint8, device=dev).view(dt)  # noqa: E731
    rows = _capi.contribution_rows(P, fwd[0], W, H, fwd[5], fwd[6], fwd[7], out=ff(torch.int64, P, 16).view(P, 2))
    out = dict(n_touched=ff(torch.int32, 4 * P), weight_sum=ff(torch.float32, 4 * P), weight_max=ff(torch.float32, 4 * P),
               mask=ff(torch.uint8, P))
    if P:
        _capi.contribution_finish(rows, min_pixels, min_weight, **out)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(rows=rows, radii=fwd[4].cpu().numpy())
    return fwd, res


def _check_weights(got, r):
    amb = 0.99 * (r["hi"] - r["lo"])
    ds = np.abs(got["weight_sum"].astype(np.float64) - r["wsum64"])
    dm = np.abs(got["weight_max"].astype(np.float64) - r["wmax64"])
    sharp = r["hi"] == r["lo"]
    print("worst |d| / f64 on unambiguous rows: weight_sum %.3e  weight_max %.3e  (bar %.3e)"
          % (CR.worst_ratio(got["weight_sum"][sharp], r["wsum64"][sharp]),
             CR.worst_ratio(got["weight_max"][sharp], r["wmax64"][sharp]), CR.B))
    assert (ds <= CR.B * r["wsum64"] + 2.0 ** -33 * r["tiles"] + amb).all(), float((ds - amb).max())
    assert (dm <= CR.B * r["wmax64"] + amb).all(), float((dm - amb).max())


# ---- 1. against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CR.SCENES)
def test_counts_and_weights_equal_the_reference(cfg, gpu_device):
    sc, fr, r = _reference(cfg)
    _, got = _run(sc, gpu_device)
    assert np.array_equal(got["radii"], fr.radii)
    n = got["n_touched"].astype(np.int64)
    assert ((r["lo"] <= n) & (n <= r["hi"])).all()       # equality on every unambiguous row
    hidden = got["radii"] <= 0
    assert not n[hidden].any()
    assert not got["weight_sum"][hidden].view(np.int32).any() and not got["weight_max"][hidden].view(np.int32).any()
    _check_weights(got, r)
    assert np.array_equal(got["mask"], (n >= 1).astype(np.uint8))
    # the feature's point: rows the rasterizer calls visible that put nothing into any pixel
    assert int(((got["radii"] > 0) & (n == 0)).sum()) >= int(((fr.radii > 0) & (r["hi"] == 0)).sum())


# ---- 2. occlusion and termination ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("opacity", [1.0, 0.95])
def test_rows_behind_an_opaque_stack_touch_nothing(opacity, gpu_device):
    N = 8
    sc = CR.stack_scene(N, opacity)
    fr = O.forward(sc)
    K = int(fr.n_contrib.max())                          # T falls below 1e-4 behind row K - 1
    assert 1 <= K < N and K == (1 if opacity == 1.0 else 3)
    fwd, got = _run(sc, gpu_device)
    v = G.state_views(fwd[5], fwd[6], fwd[7], N, fwd[0], 16, 16)
    assert int(v["n_contrib"].max()) == K and (got["radii"] > 0).all()
    assert (got["n_touched"][:K] == 256).all() and not got["n_touched"][K:].any()
    assert not got["weight_sum"][K:].any() and not got["weight_max"][K:].any()
    # mask_visible semantics: the mask differs from radii > 0 exactly on the occluded rows
    assert np.array_equal(np.flatnonzero(got["mask"] != (got["radii"] > 0)), np.arange(K, N))
    if opacity != 1.0:   # (alpha = 0.99 sits on the T < 1e-4 cut: every pixel fragile, the weights have no reference)
        _check_weights(got, CR.per_gaussian(fr))


def test_a_stack_opaque_in_the_middle_counts_only_the_open_pixels(gpu_device):
    """The pixels of one tile stop at different list positions (the middle after three entries, the border never): the
    walk is bounded by the tile's longest prefix, so only the per-pixel `position < n_contrib` cut keeps a stopped pixel
    from taking the entries behind its own."""
    sc = CR.stack_scene(8, 0.95, sigma_px=6.0)
    fr = O.forward(sc)
    r = CR.per_gaussian(fr)
    assert fr.fragile.sum() == 0 and fr.n_contrib.min() == 3 and fr.n_contrib.max() == 8
    assert r["lo"].tolist() == [256, 256, 256, 244, 224, 212, 196, 180]
    _, got = _run(sc, gpu_device)
    assert got["n_touched"].tolist() == r["lo"].tolist()
    _check_weights(got, r)


# ---- 3. sub-chunk seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 129, 257])
def test_a_transparent_stack_across_sub_chunk_seams(N, gpu_device):
    sc = CR.stack_scene(N, 0.02)
    fr = O.forward(sc)
    r = CR.per_gaussian(fr)
    assert fr.fragile.sum() == 0 and (r["lo"] == 256).all()
    _, got = _run(sc, gpu_device)
    assert (got["n_touched"] == 256).all()
    assert (np.diff(got["weight_sum"]) < 0).all() and (np.diff(got["weight_max"]) < 0).all()
    _check_weights(got, r)


# ---- 4. partial tiles -----------------------------------------------------------------------------------------------------
def test_a_splat_on_the_partial_corner_tile_is_clipped_to_the_image(gpu_device):
    sc = CR.splat_scene(70, 50, [[66.3, 48.2]], [2.0], 1.7, 0.8)
    fr = O.forward(sc)
    n_in, w_in, margin = CR.ellipse_pixels(fr, 0)
    n_all = CR.ellipse_pixels(fr, 0, clip=False)[0]
    assert margin > 1e-3 and 0 < n_in < n_all            # the footprint leaves the image on two sides
    _, got = _run(sc, gpu_device)
    assert int(got["n_touched"][0]) == n_in
    assert abs(float(got["weight_sum"][0]) - w_in) <= CR.B * w_in + 2.0 ** -33 * 4


# ---- 5. invariance, bit for bit -------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_binning_mode_or_the_run(gpu_device):
    sc, _, _ = _reference(CR.SCENES[2])
    _, a = _run(sc, gpu_device)
    _, b = _run(sc, gpu_device, ref_rects=True)
    _, c = _run(sc, gpu_device)
    assert a["rows"].any() and torch.equal(a["rows"], b["rows"]) and torch.equal(a["rows"], c["rows"])


def test_near_far_frames_equal_one_chain_frames(gpu_device):
    dev = gpu_device
    sc = S.make_scene(60_000, 640, 400, 16, sh_degree=0)   # the scene of tests/test_gpu_parity.py's near/far test
    sc["means3D"][:40, 2] = 1.0
    sc["means3D"][:40, :2] *= 0.3
    sc["scales"][:40] = 0.29
    sc["opacities"][:40] = 0.95
    try:
        for near_entries in (4, 64):
            G.set_binning_capacity_hint(0)
            _, one = _run(sc, dev)                          # synchronous, one chain
            assert not G.last_near_far()[0]
            G.set_near_far_hints(near_entries, None)
            _, two = _run(sc, dev, near_far=True)           # speculative, near/far
            torch.cuda.synchronize()
            split, n_near, n_far = G.last_near_far()
            assert split and n_near > 0 and n_far > 0
            assert one["rows"].any() and torch.equal(one["rows"], two["rows"])
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


def test_an_empty_model_and_an_empty_frame_give_zeros(gpu_device):
    sc = CR.splat_scene(33, 17, np.zeros((0, 2)), np.zeros(0), 1.0, 0.5)
    _, got = _run(sc, gpu_device)
    assert got["rows"].shape == (0, 2) and got["n_touched"].size == 0
    sc = CR.scene(50, 33, 17, 3, 0)
    sc["means3D"][:, 2] = -np.abs(sc["means3D"][:, 2]) - 1.0   # everything behind the camera: R == 0
    fwd, got = _run(sc, gpu_device)
    assert int(fwd[0]) == 0 and not (got["radii"] > 0).any()
    assert not got["rows"].any() and not got["n_touched"].any() and not got["mask"].any()
    assert not got["weight_sum"].view(np.int32).any() and not got["weight_max"].view(np.int32).any()


# ---- 6. statistics ---------------------------------------------------------------------------------------------------------
def test_two_views_fold_into_the_statistics(gpu_device):
    dev = gpu_device
    P, W, H = 300, 70, 50
    stats = torch.zeros((P, 3), device=dev)
    views = []
    for yaw in (0.0, 7.0):
        sc = S.make_scene(P, W, H, 11, sh_degree=0, yaw_deg=yaw)
        _, fwd = hip_forward(sc, dev, debug=False)
        views.append(G.contribution(fwd, P, W, H, stats=stats))
    a, b = views
    assert (a.n_touched > 0).any() and not torch.equal(a.n_touched, b.n_touched)
    assert torch.equal(stats[:, 0], a.weight_sum + b.weight_sum)
    assert torch.equal(stats[:, 1], (a.n_touched > 0).float() + (b.n_touched > 0).float())
    assert torch.equal(stats[:, 2], torch.maximum(a.weight_max, b.weight_max))
    only = G.contribution(fwd, P, W, H, stats=stats.clone(), want=())      # statistics alone
    assert only.n_touched is None and only.mask is None and only.rows.shape == (P, 2)


def _model(dev, P=300):
    g = S.make_gaussians(P, 11, 0, aspect=70 / 50)
    m = G.GrowableGaussians(512, 1, dev)
    m.add_new_pointcloud(torch.from_numpy(g["means3D"]).to(dev), (torch.eye(3, device=dev) * 1e-4).expand(P, 3, 3).contiguous(),
                         torch.full((P, 3), 128.0, device=dev))
    with torch.no_grad():
        m._features_dc[:] = torch.from_numpy(g["shs"][:, :1]).to(dev)
        m._scaling[:] = torch.from_numpy(np.log(g["scales"])).to(dev)
        m._rotation[:] = torch.from_numpy(g["rotations"]).to(dev)
        m._opacity[:] = torch.from_numpy(np.log(g["opacities"] / (1 - g["opacities"]))).to(dev)
    return m


def test_model_statistics_follow_prune_and_growth(gpu_device):
    dev = gpu_device
    m = _model(dev)
    P = m.P
    assert m.contribution_stats() is None
    m.enable_contribution_stats()
    cam = G.Camera(np.eye(3), np.zeros(3), np.radians(60.0), 2 * np.arctan(np.tan(np.radians(30.0)) * 50 / 70), 70, 50, device=dev)
    bg = torch.ones(3, device=dev)
    color, depth, acc, radii, c = G.render_contribution(cam, m, bg, min_pixels=5, stats=True)
    assert color.shape == (3, 50, 70) and radii.shape == (P,) and c.n_touched.shape == (P,)
    assert torch.equal(c.mask, (c.n_touched >= 5).to(torch.uint8))
    stats = m.contribution_stats().clone()
    assert torch.equal(stats[:, 0], c.weight_sum) and torch.equal(stats[:, 1], (c.n_touched > 0).float())
    # the mask goes straight into the covisibility records
    vis = G.KeyframeVisibility(P, device=dev)
    vis.record(c.mask)
    assert torch.equal(vis.bits[0], G.visibility_pack((c.n_touched >= 5)))
    # low contributors -> prune(drop=): exactly the marked rows leave, the statistics follow the survivors
    drop = G.low_contribution(stats, 0.05, min_views=1)
    assert 0 < int(drop.sum()) < P and torch.equal(drop.bool(), (stats[:, 1] >= 1) & (stats[:, 2] < 0.05))
    out = m.prune(min_opacity=0.0, max_scale=1e30, drop_nonfinite=False, drop=drop)
    assert torch.equal(out["reasons"] != 0, drop.bool()) and out["P_after"] == P - int(drop.sum()) == m.P
    assert torch.equal(m.contribution_stats(), stats[drop == 0])
    assert not m._cstats[m.P:].any()
    # growth: appended rows start at zero, the old rows keep theirs
    kept = m.contribution_stats().clone()
    m.enable_density_stats()
    m._stats[:10] = torch.tensor([1.0, 1.0, 0.0], device=dev)
    d = m.densify(0.5, 1e9)
    assert d["n_new"] == 10 and m.P == kept.shape[0] + 10
    assert torch.equal(m.contribution_stats()[:-10], kept) and not m.contribution_stats()[-10:].any()
    lo, hi = m.add_new_pointcloud(torch.rand(600, 3, device=dev), (torch.eye(3, device=dev) * 1e-4).expand(600, 3, 3).contiguous(),
                                  torch.full((600, 3), 128.0, device=dev))
    assert hi > 512 and torch.equal(m.contribution_stats()[:kept.shape[0]], kept) and not m.contribution_stats()[lo:].any()
    m.reset_contribution_stats()
    assert not m.contribution_stats().any()


# ---- 7. against the existing backward ------------------------------------------------------------------------------------
def test_weight_sum_equals_the_unit_upstream_backward(gpu_device):
    dev = gpu_device
    sc = dict(_reference(CR.SCENES[2])[0])
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    sc["colors_precomp"] = np.random.default_rng(7).uniform(0, 1, (P, 3)).astype(np.float32)
    sc["shs"] = None
    t, fwd = hip_forward(sc, dev, debug=False)
    c = G.contribution(fwd, P, W, H)
    dpix = np.zeros((3, H, W), np.float32)
    dpix[0] = 1.0
    g = hip_backward(sc, t, fwd, dpix, np.zeros((1, H, W), np.float32), dev, debug=False)
    grad_close(c.weight_sum.cpu().numpy(), g["dL_dcolors"][:, 0], "weight_sum")
