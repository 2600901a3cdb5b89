"""Sweep admission (csrc/seed.hip, include/gsraster.h gsr_sweep_admit): which points of a LiDAR sweep does the map, as
a keyframe renders it, not explain yet -- and what colour and size is each of them.  The producer-side step in front of
GrowableGaussians.add_new_pointcloud; GrowableGaussians.add_unexplained chains the two."""
from collections import namedtuple

import torch

from . import _capi
from .loss import _per_channel

# reason codes of Admitted.reasons and the order of Admitted.counts
ADMITTED, OUT, OCCLUDED, EXPLAINED, BEHIND, DUPLICATE = range(6)

Admitted = namedtuple("Admitted", "xyz covs rgbs index pixel z counts reasons")
Admitted.__doc__ = """What admit_sweep returns.  xyz [m,3], covs [m,3,3], rgbs [m,3] (0..255; None without an image):
the arguments of add_new_pointcloud; index [m] int32: the admitted points' rows in the sweep, ascending; pixel [m] int32
(iy W + ix) and z [m]: where the keyframe sees them; counts: six host ints {admitted, out, occluded, explained, behind,
duplicate} that sum to n; reasons: uint8 [n] on the device (want_reasons) or None."""


@torch.no_grad()
def admit_sweep(points_world, T_cw, K, height, width, *, depth_tol, occlusion_tol, depth=None, acc=None, image=None,
                lidar_depth=None, covs=None, exposure=None, log_gain=False, acc_min=0.5, occlusion_radius=1,
                footprint=1.0, min_depth=0.2, max_depth=float("inf"), one_per_pixel=True, want_reasons=False):
    """The points of a sweep that the keyframe's render does not explain, compacted in input order.

    points_world: [n,3] f32 on the device; T_cw: 3x4 or 4x4 on the host ([R | t], x_c = R x_w + t: `world_to_camera`),
    K: 3x3 (`raster_K`), the convention of `lidar_depth_image`: pixel (u, v) is the render's pixel (u, v).
    A point is dropped, in this order, when
      it is not in the view (the drop rule of `lidar_depth_image`, min_depth and max_depth included);
      lidar_depth (the sweep's own `lidar_depth_image`) holds a return nearer by more than occlusion_tol * z within
        occlusion_radius pixels: the point is seen through a gap of a nearer surface;
      depth and acc (the render's second and third outputs, given together) show a silhouette (acc >= acc_min) whose
        depth depth / acc is within depth_tol * z of z (explained) or in front of it (behind: the map's floaters'
        business, not the sweep's).  A point IN FRONT of the rendered surface by more than depth_tol * z stays;
      one_per_pixel and a nearer point (the lower row among equal z) of the sweep claims its pixel.
    The two tolerances have no default: they are the caller's policy.  covs: the sweep's covariances [n,3,3], gathered;
    without them sigma^2 I with sigma = footprint * z * 2 / (fx + fy), the point's pixel footprint.  image: the
    keyframe's [3,H,W] in 0..1; sampled bilinearly, with exposure ([3,2] rows (g, b), or [2]; log_gain as the exposure
    loss reads it) inverted, times 255.  ONE host wait: the read of the counts.  Returns `Admitted`."""
    pts = points_world.contiguous()
    if exposure is not None:
        exposure = _per_channel(exposure.detach(), 3, log_gain).contiguous()
    c = lambda t: None if t is None else t.detach().contiguous()  # noqa: E731
    out, counts, reasons = _capi.sweep_admit(
        pts, T_cw, K, height, width, depth_tol, occlusion_tol, depth=c(depth), acc=c(acc), image=c(image),
        lidar_depth=c(lidar_depth), covs=c(covs), exposure=exposure, acc_min=acc_min,
        occlusion_radius=occlusion_radius, footprint=footprint, min_depth=min_depth, max_depth=max_depth,
        one_per_pixel=one_per_pixel, want_reasons=want_reasons)
    counts = tuple(int(v) for v in counts.tolist())   # the one host wait
    m = counts[0]
    return Admitted(out["xyz"][:m], out["covs"][:m].view(m, 3, 3), None if out["rgb"] is None else out["rgb"][:m],
                    out["index"][:m], out["pixel"][:m], out["z"][:m], counts, reasons)
