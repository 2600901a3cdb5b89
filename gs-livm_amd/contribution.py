"""Per-Gaussian blend contribution of a forward: pixels touched, summed and largest blend weight (include/gsraster.h,
csrc/contrib.hip; the walk is csrc/render.hip's k_contribution_tile).

`radii > 0` says that a Gaussian is in the frustum, not scale-culled and non-degenerate -- not that it put anything into a
pixel: a splat behind a wall of opaque ones has radii > 0 and contributes nothing.  MonoGS builds covisibility and pruning
on `n_touched`, the number of pixels a Gaussian contributed to; the reference's rasterizer has no such output.  Here a
forward-only pass walks each tile's sorted list exactly as the blend did and reduces, per Gaussian, over the pixels that
took the splat: their number, the sum of alpha * T and its maximum.  Integer atomics throughout: bitwise reproducible.

The mask goes straight into `KeyframeVisibility.record(mask)` / `visibility_pack(mask)`; the sweep statistics
{weight_sum_total, views, weight_max} follow a `GrowableGaussians` through prune and growth once
`enable_contribution_stats()` was called; `low_contribution(stats, ...)` makes a drop mask for `prune(drop=)`.  Which
thresholds, which views and when to prune stays with the caller.
"""
import math
from typing import NamedTuple, Optional

import torch

from . import _capi

WANT = ("n_touched", "weight_sum", "weight_max", "mask")


class Contribution(NamedTuple):
    """n_touched [P] int32, weight_sum / weight_max [P] float32, mask [P] uint8 = (n_touched >= min_pixels and
    weight_max >= min_weight); what was not asked for is None.  rows: the integer frame rows, [P, 2] int64 =
    {wsum_fx, pixels | wmax_bits << 32}."""
    n_touched: Optional[torch.Tensor]
    weight_sum: Optional[torch.Tensor]
    weight_max: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]
    rows: torch.Tensor


def contribution(fwd, P, W, H, min_pixels=1, min_weight=0.0, stats=None, want=WANT):
    """The contribution of the forward `fwd` -- the tuple `rasterize_forward` returned -- in three launches (zero fill,
    walk, finish).  stats: a contiguous [P, 3] float32 device tensor {weight_sum_total, views, weight_max} the view is
    folded into in place (GrowableGaussians.contribution_stats()), or None.  want: which of n_touched / weight_sum /
    weight_max / mask to produce.  Returns a Contribution."""
    unknown = set(want) - set(WANT)
    if unknown:
        raise ValueError("contribution: unknown output %s" % sorted(unknown))
    if not want and stats is None:
        raise ValueError("contribution: nothing is asked for")
    R, geom, binning, img = fwd[0], fwd[5], fwd[6], fwd[7]
    P = int(P)
    dev = fwd[1].device
    rows = _capi.contribution_rows(P, R, W, H, geom, binning, img)
    mk = lambda name, dt: torch.empty(P, dtype=dt, device=dev) if name in want else None  # noqa: E731
    out = dict(n_touched=mk("n_touched", torch.int32), weight_sum=mk("weight_sum", torch.float32),
               weight_max=mk("weight_max", torch.float32), mask=mk("mask", torch.uint8))
    if stats is not None and tuple(stats.shape) != (P, 3):
        raise ValueError("contribution: stats is [P, 3]")
    if P:  # (an empty model: empty outputs, nothing to launch)
        _capi.contribution_finish(rows, min_pixels, min_weight, stats=stats, **out)
    return Contribution(rows=rows, **out)


def forward_of(viewpoint_camera, gaussian_model, bg_color, scaling_modifier=1.0, override_color=None):
    """A forward of `gaussian_model` from `viewpoint_camera` for the passes that walk its tile lists afterwards
    (contribution, attribute blend): -> (the tuple `rasterize_forward` returned, P, W, H, the activated (xyz, scaling,
    rotation) it rendered).  Call under no_grad."""
    cam = viewpoint_camera
    dev = gaussian_model.Get_xyz().device
    if hasattr(gaussian_model, "activated"):
        means3D, opacity, scales, rotations, shs = gaussian_model.activated()
    else:
        means3D, opacity = gaussian_model.Get_xyz(), gaussian_model.Get_opacity()
        scales, rotations, shs = gaussian_model.Get_scaling(), gaussian_model.Get_rotation(), gaussian_model.Get_features()
    empty = torch.empty(0, device=dev)
    colors = empty
    if override_color is not None and override_color.numel():
        colors, shs = override_color.contiguous(), empty
    H, W = int(cam.Get_image_height()), int(cam.Get_image_width())
    fwd = _capi.rasterize_forward(
        bg_color.to(dev), means3D.contiguous(), colors, opacity.contiguous(), scales.contiguous(),
        rotations.contiguous(), float(scaling_modifier), empty, cam.Get_world_view_transform().contiguous(),
        cam.Get_full_proj_transform().contiguous(), math.tan(cam.Get_FoVx() * 0.5), math.tan(cam.Get_FoVy() * 0.5), H, W,
        shs.contiguous(), int(gaussian_model.Get_max_sh_degree()), cam.Get_camera_center().contiguous(), False, False)
    return fwd, int(means3D.size(0)), W, H, (means3D, scales, rotations)


@torch.no_grad()
def render_contribution(viewpoint_camera, gaussian_model, bg_color, scaling_modifier=1.0, override_color=None,
                        min_pixels=1, min_weight=0.0, stats=None, want=WANT):
    """A forward of `gaussian_model` from `viewpoint_camera` (no autograd graph) plus the contribution pass:
    -> (color [3,H,W], depth [1,H,W], depth_acc [1,H,W], radii [P] int32, Contribution).  stats=True folds the view into
    the model's own statistics (GrowableGaussians.enable_contribution_stats()); a tensor is used as given."""
    fwd, P, W, H, _ = forward_of(viewpoint_camera, gaussian_model, bg_color, scaling_modifier, override_color)
    if stats is True:
        stats = gaussian_model.contribution_stats()
        if stats is None:
            raise RuntimeError("render_contribution: call enable_contribution_stats() first")
    c = contribution(fwd, P, W, H, min_pixels, min_weight, stats, want)
    return fwd[1], fwd[2], fwd[3], fwd[4], c


def low_contribution(stats, max_weight_below, min_views=1):
    """[P] uint8 drop mask for `GrowableGaussians.prune(drop=)` from the sweep statistics [P, 3] = {weight_sum_total,
    views, weight_max}: 1 for a row that at least `min_views` views blended and whose largest weight over all of them
    stayed below `max_weight_below` (a floater or a buried Gaussian), and -- with min_views <= 0 -- also for the rows no
    view blended at all.  Plain Torch ops; the policy stays with the caller."""
    return ((stats[:, 1] >= float(min_views)) & (stats[:, 2] < float(max_weight_below))).to(torch.uint8)
