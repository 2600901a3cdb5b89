"""The scene of tests/iteration.py on the CPU, with the oracle standing in for the renders, forward only: the properties
tests/test_gpu_iteration.py relies on.  A view that saw nothing, a term whose mask is empty, a similarity point on a
decision boundary or a density-control threshold nothing crosses would let that file pass without checking much."""
import math

import numpy as np
import pytest
import torch

import delta_ref
import iteration as I
import lidar_ref
from gs_livm_amd import loss as GL

N = I.W * I.H


def _pct(x):
    """A share in whole per cent: the precision at which the scene's figures are stated (module docstring of
    tests/iteration.py)."""
    return int(round(100.0 * x))


def _masked(v):
    fr, mk = I.oracle_frames()[v], I.keep_masks()[v].numpy()
    return fr.out_depth * mk, fr.out_acc * mk


def _host_pose(v):
    rpy, T = I.POSES[v]
    import poses
    return torch.as_tensor(poses.rotation(**rpy), dtype=torch.float32), torch.as_tensor(T, dtype=torch.float32)


@pytest.mark.parametrize("v", range(3))
def test_every_view_sees_the_map(v):
    fr = I.oracle_frames()[v]
    visible = int((fr.radii > 0).sum())
    silhouette = float((fr.out_acc >= 0.5).mean())
    fragile = float((fr.fragile != 0).mean())
    print("view", v, "visible", visible, "silhouette %.4f" % silhouette, "fragile %.5f" % fragile)
    assert 521 <= visible <= 584
    assert 48 <= _pct(silhouette) <= 50
    assert fragile <= 0.0003
    assert (I.W + 15) // 16 == 5 and (I.H + 15) // 16 == 4 and I.W % 16 and I.H % 16


@pytest.mark.parametrize("v", range(3))
def test_lidar_term_supervises_a_third_of_each_view(v):
    D, A = _masked(v)
    zl, kept, hit, _ = lidar_ref.image64(I.sweep(), I.world_to_camera(v), I.raster_K(), I.H, I.W, lidar_ref.MIN_DEPTH,
                                         float("inf"))
    zl = zl.astype(np.float32)
    t = lidar_ref.loss_ops(D[0], A[0], zl, I.ACC_MIN, I.LAMBDAS["lidar"])
    b = lidar_ref.bars(dict(t, depth=D[0], acc=A[0], lidar=zl, acc_min=I.ACC_MIN, lam=I.LAMBDAS["lidar"]))
    share = float(t["share"])
    print("view", v, "supervised %.4f" % share, "sign-fragile", int(b["F3"].sum()), "hit", hit)
    assert 34 <= _pct(share) <= 37
    assert int(b["F3"].sum()) == 0 <= 0.01 * N
    assert bool(t["grad_depth"].any()) and bool(t["grad_acc"].any())


@pytest.mark.parametrize("pair", I.PAIRS)
def test_delta_term_reaches_both_views(pair):
    s, r = pair
    (Ds, As), (Dr, Ar) = _masked(s), _masked(r)
    T = GL.delta_pose(*_host_pose(s), *_host_pose(r))
    K = I.raster_K()
    x = dict(depth_src=Ds[0], acc_src=As[0], depth_ref=Dr[0], acc_ref=Ar[0], inv_K_src=np.linalg.inv(K).astype(np.float32),
             K_ref=K.astype(np.float32), T_rel=T.numpy(), lam=I.LAMBDAS["delta"], H=I.H, W=I.W)
    ref = delta_ref.evaluate(x)
    share, kept = float(ref["truth"]["share"]), float(ref["keep"]["grad_src"].double().mean())
    print("pair", pair, "mask share %.4f" % share, "fragile %.5f" % ref["fragile_share"], "grad_src kept %.5f" % kept)
    assert 25 <= _pct(share) <= 30
    assert ref["fragile_share"] <= 0.01                       # delta_ref's own condition
    assert round(100.0 * kept, 1) >= 99.9
    assert bool(ref["truth"]["grad_src"].any()) and bool(ref["truth"]["grad_ref"].any())


def test_similarity_points_keep_their_margins():
    sc = I.scene()
    lo, hi = I.SEL_ROWS
    pts = I.simi_points()
    allp = np.concatenate([pts[k].numpy() for k in sorted(pts)])
    r = float(sc["scales"][lo:hi].astype(np.float64).mean())
    d, gap, clamp = I.simi_margins(allp, sc["means3D"][lo:hi], r)
    inside = int((d < r).sum())
    print("points", len(allp), "inside r", inside, "smallest gap %.2e clamp margin %.2e" % (gap.min(), clamp.min()))
    assert len(allp) == I.M_POINTS == 257 and set(pts) <= set(I.VOXEL_KEYS)
    assert gap.min() >= I.MARGIN and clamp.min() >= I.MARGIN
    assert 10 <= inside <= len(allp) - 100          # both sides of the clamp are populated
    assert hi - lo == 16 * len(I.VOXEL_KEYS)


def test_weights_hide_no_missing_factor():
    for k, w in I.WEIGHTS.items():
        w32 = float(np.float32(w))
        assert w32 != 1.0 and math.frexp(w32)[0] != 0.5, k     # neither 1 nor a power of two
    assert len(set(I.WEIGHTS.values())) == len(I.WEIGHTS)


def test_targets_differ_per_view_and_stay_in_range():
    gts = I.targets()
    for v, gt in enumerate(gts):
        assert tuple(gt.shape) == (3, I.H, I.W) and float(gt.min()) >= 0.0 and float(gt.max()) <= 1.0
        own = torch.from_numpy(I.oracle_frames()[v].out_color)
        assert float((gt - own).abs().mean()) > 1e-3           # there is something to learn
    assert not torch.equal(gts[0], gts[1])


def test_prune_has_rows_to_drop():
    """Rows no view sees (the 2 % behind the cameras) and rows beyond the scale cull (1 % at three times the scale):
    the prune between iterations 2 and 3 changes the row count whatever the optimiser did to the rest."""
    seen = np.zeros(I.P0, bool)
    for fr in I.oracle_frames():
        seen |= fr.radii > 0
    big = (I.scene()["scales"].max(1) > 0.3 * 1.05)
    print("unseen rows", int((~seen).sum()), "beyond the scale cull", int(big.sum()))
    assert int((~seen).sum()) >= 5 and int(big.sum()) >= 1


def test_density_thresholds_move_the_row_count():
    """The statistics densify reads, predicted in float64 at the starting state: the image gradients of the composed loss
    (iteration.image_anchor on the oracle's frames), depth_ref.render64 per render for dL/dmean2D, |.xy| averaged over the
    renders that see a row, as k_density_accumulate does.  The scripted thresholds must leave candidates on both sides
    of the size threshold, and must not take every row, with half an order of magnitude to spare either way."""
    import depth_ref
    frames = I.oracle_frames()
    lidar = [torch.from_numpy(lidar_ref.image64(I.sweep(), I.world_to_camera(v), I.raster_K(), I.H, I.W, lidar_ref.MIN_DEPTH,
                                                float("inf"))[0].astype(np.float32)) for v in range(3)]
    K = I.raster_K()
    st = dict(w={k: torch.tensor(w, dtype=torch.float32) for k, w in I.WEIGHTS.items()}, masks=list(I.keep_masks()),
              gts=list(I.targets()), lidar=lidar, K=K, iK=np.linalg.inv(K).astype(np.float32))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    rec = dict(images=[[f(frames[ci].out_color), f(frames[ci].out_depth), f(frames[ci].out_acc)] for ci in I.RENDERS],
               exposures=[torch.tensor(e, dtype=torch.float32) for e in I.EXPOSURES],
               T_rel=[GL.delta_pose(*_host_pose(s), *_host_pose(r)) for s, r in I.PAIRS],
               terms=dict(simi=torch.tensor(0.0)), total=torch.tensor(0.0))
    _, fragile, truth = I.image_anchor(st, rec, want_truth=True)
    assert max(fragile.values()) <= 0.01
    grad_sum, views = np.zeros(I.P0), np.zeros(I.P0)
    zero = np.zeros((1, I.H, I.W), np.float32)
    for r, ci in enumerate(I.RENDERS):
        g_c, g_d, g_a = (zero if t is None else t.reshape(-1, I.H, I.W).numpy().astype(np.float32) for t in truth[r])
        ref = depth_ref.render64(I.view_scene(ci), frames[ci], g_c, g_a, g_d)
        seen = frames[ci].radii > 0
        m2d = np.asarray(ref["dL_dmeans2D"], np.float64)
        grad_sum += np.where(seen, np.hypot(m2d[:, 0], m2d[:, 1]), 0.0)
        views += seen
    mean = grad_sum[views > 0] / views[views > 0]
    size = I.scene()["scales"].max(1)[views > 0]
    th, sz = I.DENSIFY["grad_threshold"], I.DENSIFY["size_threshold"]
    count = lambda t: (int(((mean >= t) & (size <= sz)).sum()), int(((mean >= t) & (size > sz)).sum()))  # noqa: E731
    print("rows seen", int((views > 0).sum()), "mean-gradient quantiles", np.round(np.quantile(mean, [0.1, 0.5, 0.9]), 4),
          "(clones, splits) at the threshold", count(th), "at three times", count(3 * th), "at a third", count(th / 3))
    for t in (th, 3 * th):
        clones, splits = count(t)
        assert clones >= 2 and splits >= 2
    assert sum(count(th / 3)) < int((views > 0).sum())
