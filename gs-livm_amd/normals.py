"""Rendered normal maps and the depth-normal consistency loss (include/gsraster.h, csrc/normal.hip; the attribute walk
is csrc/render.hip's k_attribute_tile).

The voxel map seeds flat, oriented surfels and the point-to-plane loss keeps them turned towards the LiDAR points, but
nothing ties the rendered depth SURFACE to those orientations: between LiDAR returns it is free to ripple.  2DGS and
PGSR close that loop in image space and so does this module: `render_normals` blends each Gaussian's camera-facing thin
axis into a normal image with the forward's own alpha and T, and `normal_consistency_loss` holds the normals of the
rendered depth (finite differences of the back-projected depth) to it.  The loss moves depth and the silhouette -- render
the view with depth_gradient=True -- and not the rotations: the blend has no backward, the normal image is data.
`blend_attributes` is the general pass underneath: any [P, 1..4] per-Gaussian attribute, blended as the forward blends
colour.  lambda_, normal_min and jump_rel are the caller's policy.
"""
import torch

from . import _capi
from .contribution import forward_of
from .loss import world_to_camera


def blend_attributes(fwd, attributes, W, H):
    """[C, H, W] = sum over the splats each pixel took of attributes[splat] * alpha * T, for the forward `fwd` -- the
    tuple `rasterize_forward` returned.  attributes: [P, C] (or [P]) float32 on the device, C in 1..4.  No background
    term; a pixel that took nothing reads 0.  One launch, bitwise reproducible, no autograd graph."""
    attributes = attributes.detach()
    if attributes.dim() == 1:
        attributes = attributes[:, None]
    if attributes.dim() != 2 or not 1 <= int(attributes.shape[1]) <= 4:
        raise ValueError("blend_attributes: attributes is [P, C] with C in 1..4")
    R, geom, binning, img = fwd[0], fwd[5], fwd[6], fwd[7]
    return _capi.blend_attributes(int(attributes.shape[0]), R, W, H, attributes.contiguous().float(), geom, binning, img)


@torch.no_grad()
def render_attributes(viewpoint_camera, gaussian_model, bg_color, attributes, scaling_modifier=1.0,
                      override_color=None):
    """A forward of `gaussian_model` from `viewpoint_camera` (no autograd graph) plus the attribute blend:
    -> (color [3,H,W], depth [1,H,W], depth_acc [1,H,W], radii [P] int32, blended [C,H,W])."""
    fwd, P, W, H, _ = forward_of(viewpoint_camera, gaussian_model, bg_color, scaling_modifier, override_color)
    if int(attributes.shape[0]) != P:
        raise ValueError("render_attributes: one attribute row per Gaussian")
    return fwd[1], fwd[2], fwd[3], fwd[4], blend_attributes(fwd, attributes, W, H)


def surfel_normals(xyz, scaling, rotation, T_cw):
    """[P, 3]: column k* of R(q) of every row -- k* the index of its smallest ACTIVATED scale, the lowest index on a tie,
    q = (w, x, y, z) as given -- turned into camera axes by T_cw = [R | t] (host, 3x4 or 4x4: `world_to_camera`) and
    negated where it points away from the camera (n_c . p_c > 0).  One launch, no autograd graph."""
    return _capi.surfel_normals(xyz.detach().contiguous().float(), scaling.detach().contiguous().float(),
                                rotation.detach().contiguous().float(), T_cw)


@torch.no_grad()
def render_normals(viewpoint_camera, gaussian_model, bg_color, scaling_modifier=1.0):
    """A forward of `gaussian_model` from `viewpoint_camera` (no autograd graph) plus its normal map:
    -> (color [3,H,W], depth [1,H,W], depth_acc [1,H,W], radii [P] int32, normals [3,H,W]).  normals = sum n_c alpha T in
    camera axes, un-normalised -- divide by its length for unit normals, by depth_acc for the mean -- and is what
    `normal_consistency_loss` takes."""
    fwd, P, W, H, (xyz, scaling, rotation) = forward_of(viewpoint_camera, gaussian_model, bg_color, scaling_modifier)
    n = surfel_normals(xyz, scaling, rotation, world_to_camera(viewpoint_camera))
    return fwd[1], fwd[2], fwd[3], fwd[4], blend_attributes(fwd, n, W, H)


class NormalConsistencyLoss(torch.autograd.Function):
    """loss = lambda * mean over the supervised pixels of 1 - n_r . n_d as one node (csrc/normal.hip): n_r the normalised
    blended normal, n_d the normal of the rendered depth surface.  Gradients w.r.t. the rendered depth and silhouette
    only (the normal image is data, the gates are steps), scaled by the upstream scalar."""

    @staticmethod
    def forward(ctx, depth, acc, normals, fx, fy, cx, cy, acc_min, normal_min, jump_rel, lambda_):
        need_d, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        out3, gd, ga = _capi.normal_consistency_loss(depth.contiguous(), acc.contiguous(), normals.contiguous(), fx, fy,
                                                     cx, cy, acc_min, normal_min, jump_rel, lambda_,
                                                     want_grad_depth=need_d, want_grad_acc=need_a)
        ctx.grads = (gd, ga)
        ctx.parts = out3  # [loss, mean rho, supervised share] for logging
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        gd, ga = ctx.grads
        return ((gd * g if gd is not None else None), (ga * g if ga is not None else None)) + (None,) * 9


def normal_consistency_loss(depth, acc, normals, K, acc_min=0.5, *, lambda_, normal_min, jump_rel=float("inf")):
    """depth, acc: the second and third outputs of `render` ([H,W] or [1,H,W] f32 on the device, un-normalised);
    normals: the fifth output of `render_normals` of the same view; K: the 3x3 pinhole of the render, `raster_K`.
    A pixel is supervised when it and its four neighbours have acc >= acc_min, their depths differ from its own by at
    most jump_rel * z (+inf: no such gate), |normals| >= normal_min * acc and the depth surface has a normal.
    lambda_ and normal_min have no default, on purpose.  Returns the 0-dim loss."""
    K = torch.as_tensor(K).detach().cpu().double()
    return NormalConsistencyLoss.apply(depth, acc, normals.detach(), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                                       float(K[1, 2]), float(acc_min), float(normal_min), float(jump_rel),
                                       float(lambda_))


__all__ = ["blend_attributes", "render_attributes", "surfel_normals", "render_normals", "NormalConsistencyLoss",
           "normal_consistency_loss"]
