"""Host-side mirror of the reference's image loss (include/gs/gs/loss_utils.cuh) on the fused kernels of
csrc/loss.hip (SURVEY.md section 8(f) "next" row 2), and of its LiDAR similarity loss
(GaussianModel::compute_min_distance, src/gs/gaussian.cu:87-114) on those of csrc/simi.hip, and of the delta-depth
term between keyframe pairs (GaussianModel::calcDeltaSimi, src/gs/gaussian.cu:116-199, and the loop around it,
src/liw/lioOptimization.cpp:1780-1801) on those of csrc/delta.hip, and the LiDAR depth supervision of csrc/lidar.hip
(an extension: a sweep's z-buffer in a keyframe's view and the masked depth L1 of a render against it), and the weighted
photometric loss of csrc/weighted.hip (an extension: per-pixel weights, a silhouette gate and the exposure in one
term)."""
import math

import torch

from . import _capi


def reference_window_1d(window_size=11, sigma=1.5):
    """The 1-D kernel of gaussian_splatting::gaussian (loss_utils.cuh:24-31), bug for bug: the exponent uses
    floor((x - window_size) / 2), not (x - window_size // 2), so the window is NOT the centred Gaussian of the
    original SSIM code.  The 2-D window of create_window (:33-37) is the outer product of this vector."""
    g = [math.exp(-(math.floor((x - window_size) / 2.0) ** 2) / (2.0 * sigma * sigma)) for x in range(window_size)]
    t = torch.tensor(g, dtype=torch.float32)
    return t / t.sum()


class PhotometricLoss(torch.autograd.Function):
    """loss = (1 - lambda_dssim) * l1_loss(img, gt) + lambda_dssim * (1 - ssim(img, gt))
    (src/liw/lioOptimization.cpp:1705-1710); gradient w.r.t. img only (gt is data)."""

    @staticmethod
    def forward(ctx, img, gt, window11, lambda_dssim):
        out3, grad = _capi.photometric_loss(img, gt, window11.tolist(), lambda_dssim, want_grad=img.requires_grad)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0, device=img.device))
        ctx.parts = out3  # [loss, l1, ssim] for logging (the reference prints PSNR/SSIM every 50 iterations)
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad.numel() else None), None, None, None


def photometric_loss(img, gt, lambda_dssim=0.2, window11=None):
    """Drop-in for the reference's three lines at lioOptimization.cpp:1705-1710 (lambda_dssim:
    config/basic_common.yaml:63)."""
    if window11 is None:
        window11 = reference_window_1d()
    return PhotometricLoss.apply(img, gt, window11, float(lambda_dssim))


class ExposureLoss(torch.autograd.Function):
    """photometric_loss on the exposure-compensated image x' = fma(g_c, img, b_c) as one node (csrc/exposure.hip; an
    extension: the reference has no such term); gradients w.r.t. img and the [C,2] exposure (gt is data), both scaled
    by the upstream scalar."""

    @staticmethod
    def forward(ctx, img, gt, exposure, window11, lambda_dssim):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        out3, grad, grad_e = _capi.exposure_loss(img, gt, exposure, window11.tolist(), lambda_dssim, want_grad=want)
        ctx.grads = (grad, grad_e)
        ctx.parts = out3  # [loss, l1, ssim] of the compensated image, for logging
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        grad, grad_e = ctx.grads
        need_i, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        return (grad * g if need_i else None), None, (grad_e * g if need_e else None), None, None


def identity_exposure(channels=3, device=None):
    """The exposure that changes nothing: [C,2] f32 rows (g, b) = (1, 0).  A keyframe's leaf starts here."""
    e = torch.zeros((int(channels), 2), dtype=torch.float32, device=device)
    e[:, 0] = 1.0
    return e


def _per_channel(exposure, channels, log_gain=False):
    """[C,2] rows (g_c, b_c) from [C,2] or a shared [2] (expanded: autograd sums its gradient over the channels);
    log_gain: column 0 holds a with g = exp(a) (the MonoGS parametrisation), on C numbers in Torch."""
    if exposure.dim() == 1:
        exposure = exposure.expand(channels, 2)
    if log_gain:
        exposure = torch.stack((torch.exp(exposure[:, 0]), exposure[:, 1]), dim=1)
    return exposure


def exposure_photometric_loss(img, gt, exposure, lambda_dssim=0.2, window11=None, log_gain=False):
    """photometric_loss(g * img + b, gt) without the compensated image ever reaching memory: the keyframe's exposure
    ([C,2] rows (g_c, b_c), or [2] shared by the channels; f32 on the device, typically a leaf beside the pose leaf)
    absorbs the camera's auto-exposure step instead of the map.  log_gain=True reads column 0 as log g.  Returns the
    0-dim loss; gradients flow to img and exposure."""
    if window11 is None:
        window11 = reference_window_1d()
    e = _per_channel(exposure, int(img.shape[0]), log_gain)
    return ExposureLoss.apply(img, gt, e, window11, float(lambda_dssim))


class WeightedPhotometricLoss(torch.autograd.Function):
    """The photometric loss taken where the caller says: w = weights * [acc >= acc_min], every sum normalised by the
    weight sum, on x' = fma(g_c, img, b_c) when an exposure is given, as one node (csrc/weighted.hip).  Gradients
    w.r.t. img and the [C,2] exposure only (gt, weights and acc are data; the gate is a step), both scaled by the
    upstream scalar."""

    @staticmethod
    def forward(ctx, img, gt, weights, acc, acc_min, exposure, window11, lambda_dssim):
        need_e = exposure is not None and ctx.needs_input_grad[5]
        want = ctx.needs_input_grad[0] or need_e
        out6, grad, grad_e = _capi.weighted_loss(img, gt, weights, acc, acc_min, exposure, window11.tolist(),
                                                 lambda_dssim, want_grad=want)
        ctx.grads = (grad, grad_e)
        ctx.parts = out6  # [loss, l1, ssim, weight sum, mse, psnr] for logging
        return out6[0]

    @staticmethod
    def backward(ctx, g):
        grad, grad_e = ctx.grads
        need_i, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[5] and grad_e is not None
        return (grad * g if need_i else None), None, None, None, None, (grad_e * g if need_e else None), None, None


def weighted_photometric_loss(img, gt, weights=None, acc=None, acc_min=0.5, exposure=None, lambda_dssim=0.2,
                              window11=None, log_gain=False):
    """photometric_loss / exposure_photometric_loss over the pixels that carry a measurement: weights ([H,W] f32 on the
    device, finite and >= 0: an undistortion border, a sky or dynamic-object mask, a texture weight) times the gate
    [acc >= acc_min] (acc: [H,W] or [1,H,W], e.g. the silhouette `render` returns -- it is detached, the gate has no
    gradient), each optional.  L1, SSIM and the squared error are weighted per pixel and divided by the weight sum; the
    SSIM windows still see the whole images, so a zero weight does not shield a non-finite pixel from its neighbours.
    exposure: [C,2], [2] or (log_gain=True) log-gain, as in `exposure_photometric_loss`, or None.  Returns the 0-dim
    loss; `.grad_fn.parts` holds {loss, l1, ssim, weight sum, mse, psnr}.  Gradients flow to img and exposure."""
    if window11 is None:
        window11 = reference_window_1d()
    H, W = int(img.shape[1]), int(img.shape[2])
    plane = lambda t: None if t is None else t.detach().reshape(H, W)  # noqa: E731
    e = None if exposure is None else _per_channel(exposure, int(img.shape[0]), log_gain)
    return WeightedPhotometricLoss.apply(img, gt, plane(weights), plane(acc), float(acc_min), e, window11,
                                         float(lambda_dssim))


def apply_exposure(img, exposure, out=None):
    """g_c * img + b_c (one fused multiply-add per element, no graph) for evaluation and export: what a keyframe's
    learnt exposure makes of its render.  img: [C,H,W] f32 on the device; exposure: [C,2] or [2]; out: a contiguous
    tensor to write (img itself is allowed) or None."""
    with torch.no_grad():
        return _capi.apply_exposure(img.detach().contiguous(), _per_channel(exposure.detach(), int(img.shape[0])).contiguous(),
                                    out=out)


class SimilarityLoss(torch.autograd.Function):
    """loss = lambda * compute_min_distance(points, xyz[sel], scaling[sel]) (src/gs/gaussian.cu:87-114, 230-237) as
    one node; gradients w.r.t. xyz and the ACTIVATED scaling (points and sel are data).  The gradients are dense [P,3]
    tensors that are zero outside the selection, so autograd adds them to whatever else flows into `xyz` and `scaling`:
    the rasterizer's gradients, on either activation path of model.py (FusedActivations runs its chain rule on the
    sum, the stashing tail parks the sum in `_act_grads`)."""

    @staticmethod
    def forward(ctx, points, sel, xyz, scaling, lambda_):
        xyz_c, scaling_c = xyz.contiguous(), scaling.contiguous()
        need_x, need_s = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gx = torch.zeros_like(xyz_c) if need_x else None
        gs = torch.zeros_like(scaling_c) if need_s else None
        out3 = _capi.similarity_loss(points.contiguous(), sel.contiguous(), xyz_c, scaling_c, lambda_, gx, gs)
        ctx.grads = (gx, gs)
        ctx.parts = out3  # [loss, mean clamped distance, r] for logging
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        gx, gs = ctx.grads
        return None, None, (gx * g if gx is not None else None), (gs * g if gs is not None else None), None


def similarity_loss(points, sel, xyz, scaling, lambda_=0.2):
    """Drop-in for `lambda * compute_min_distance(selected_points, xyz_for_loss, scale_for_loss)`
    (src/gs/gaussian.cu:237; lambda_depth_simi: config/basic_common.yaml:64) without the two index_select: points
    [m,3] f32 and sel [n] int32 (ascending unique rows) come from `VoxelIndex.select` (model.py), xyz is the model's
    _xyz and scaling its activated scales.  Returns the 0-dim loss."""
    return SimilarityLoss.apply(points, sel, xyz, scaling, float(lambda_))


class SurfelPlaneLoss(torch.autograd.Function):
    """The point-to-plane term on oriented surfels (csrc/surfel.hip; an extension, the reference has none) as one
    node; gradients w.r.t. xyz, the ACTIVATED scaling and the ACTIVATED rotation (points and sel are data).  As
    SimilarityLoss, the gradients are dense tensors that are zero outside the selection, allocated only for the inputs
    that need one, so autograd adds them to the rasterizer's on either activation path of model.py."""

    @staticmethod
    def forward(ctx, points, sel, xyz, scaling, rotation, lambda_, huber, max_dist, lambda_flat):
        xyz_c, scaling_c, rotation_c = xyz.contiguous(), scaling.contiguous(), rotation.contiguous()
        need = ctx.needs_input_grad[2:5]
        gx, gs, gr = (torch.zeros_like(t) if want else None for t, want in zip((xyz_c, scaling_c, rotation_c), need))
        out4 = _capi.surfel_plane_loss(points.contiguous(), sel.contiguous(), xyz_c, scaling_c, rotation_c, lambda_,
                                       huber, max_dist, lambda_flat, gx, gs, gr)
        ctx.grads = (gx, gs, gr)
        ctx.parts = out4  # [loss, mean rho, mean thinnest scale, share of points inside max_dist] for logging
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(t * g if t is not None else None for t in ctx.grads) + (None, None, None, None)


def surfel_plane_loss(points, sel, xyz, scaling, rotation, lambda_, huber=0.0, max_dist=float("inf"), lambda_flat=0.0):
    """lambda_ * mean_i [d_i <= max_dist] rho(n_j . (p_i - xyz_j)) + lambda_flat * mean_j min_k scaling[j][k]: every
    point against the thinnest axis n_j of its nearest selected Gaussian j (include/gsraster.h,
    gsr_surfel_plane_loss).  points [m,3] f32 and sel [n] int32 come from `VoxelIndex.select`; xyz is the model's _xyz,
    scaling and rotation the activated values of the iteration's `activated()`.  `lambda_` has no default: the term is
    an extension without a reference value.  Returns the 0-dim loss."""
    return SurfelPlaneLoss.apply(points, sel, xyz, scaling, rotation, float(lambda_), float(huber), float(max_dist),
                                 float(lambda_flat))


class DeltaDepthLoss(torch.autograd.Function):
    """loss = lambda * mean|inv_depth(calcDeltaSimi(src, ref)) mask - inv_depth(depth_ref) mask|
    (src/liw/lioOptimization.cpp:1780-1801) as one node; gradients w.r.t. the two rendered DEPTH images only (the
    silhouettes enter through comparisons; the matrices are data), scaled by the upstream scalar.  In the reference this
    term never moves a Gaussian, because its rasterizer's backward drops dL/ddepth; here it does when the views were
    rendered with depth_gradient=True."""

    @staticmethod
    def forward(ctx, depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, lambda_):
        need_s, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        out3, _, gs, gr = _capi.delta_depth_loss(depth_src.contiguous(), acc_src.contiguous(), depth_ref.contiguous(),
                                                 acc_ref.contiguous(), inv_K_src, K_ref, T_rel, lambda_,
                                                 want_warped=False, want_grad_src=need_s, want_grad_ref=need_r)
        ctx.grads = (gs, gr)
        ctx.parts = out3  # [loss, mean gap, share of unmasked pixels] for logging
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        gs, gr = ctx.grads
        return ((gs * g if gs is not None else None), None, (gr * g if gr is not None else None), None, None, None,
                None, None)


def delta_depth_loss(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, lambda_=0.2):
    """Drop-in for the body of the loop at lioOptimization.cpp:1780-1801 (lambda_delta_depth_simi:
    config/basic_common.yaml:65): depth_* / acc_* are the rendered depth and silhouette (`depth_sol`) of the history
    keyframe and its successor, [H,W] or [1,H,W] f32 on the device; inv_K_src, K_ref: 3x3 on the host; T_rel: what
    `delta_pose` returns.  Returns the 0-dim loss."""
    return DeltaDepthLoss.apply(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, float(lambda_))


def delta_pose(R_src, t_src, R_ref, t_ref):
    """T_rel = T_ref T_src^-1 as calcDeltaSimi builds it (src/gs/gaussian.cu:138-162), [3,4] float32 on the host.
    R_* are what the cameras' Get_R() return.  The reference reads Eigen's COLUMN-major Matrix3f through from_blob as
    ROW-major (:138-151), so the 4x4 matrices it composes hold the TRANSPOSE of Get_R(); that is reproduced here.
    Computed in float64 and rounded once."""
    def T(R, t):
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3] = torch.as_tensor(R, dtype=torch.float64).reshape(3, 3).t()
        m[:3, 3] = torch.as_tensor(t, dtype=torch.float64).reshape(3)
        return m
    rel = T(R_ref, t_ref) @ torch.linalg.inv(T(R_src, t_src))
    return rel[:3].to(torch.float32)


def lidar_depth_image(points_world, T_cw, K, height, width, min_depth=0.2, max_depth=float("inf"), want_counts=False):
    """The LiDAR depth image of a keyframe, built once when the keyframe is created: the smallest camera-frame z of
    the sweep's points per pixel, 0 where none lands ([H,W] f32 on the device of points_world [n,3]).  T_cw: 3x4 or 4x4
    ([R | t], x_c = R x_w + t: `world_to_camera`), K: 3x3 (`raster_K`), both on the host.  min_depth = 0.2 is the
    rasterizer's near cull.  want_counts adds an int32 device tensor {points kept, pixels hit}."""
    return _capi.lidar_depth_image(points_world.contiguous(), T_cw, K, height, width, min_depth, max_depth,
                                   want_counts)


class LidarDepthLoss(torch.autograd.Function):
    """loss = lambda * mean over the supervised pixels of |depth / acc - lidar_depth| as one node (csrc/lidar.hip);
    supervised: lidar_depth > 0 and acc >= acc_min.  Gradients w.r.t. the rendered depth and silhouette only (the
    LiDAR image is data), scaled by the upstream scalar.  They move the Gaussians when the view was rendered with
    depth_gradient=True; without it only the silhouette route does."""

    @staticmethod
    def forward(ctx, depth, acc, lidar_depth, acc_min, lambda_):
        need_d, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        out3, gd, ga = _capi.lidar_depth_loss(depth.contiguous(), acc.contiguous(), lidar_depth.contiguous(), acc_min,
                                              lambda_, want_grad_depth=need_d, want_grad_acc=need_a)
        ctx.grads = (gd, ga)
        ctx.parts = out3  # [loss, mean |depth error| in metres, supervised share] for logging
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        gd, ga = ctx.grads
        return (gd * g if gd is not None else None), (ga * g if ga is not None else None), None, None, None


def lidar_occlusion_filter(lidar_depth, radius, tol, want_counts=False):
    """The LiDAR depth image without the returns seen through the gaps of a nearer surface: a pixel whose window of
    `radius` pixels (0..3) holds a return nearer by more than tol * z is set to 0, every other pixel keeps its bits
    (0, negatives and NaN become 0).  The rule of sweep admission's OCCLUDED code, applied to the image the depth loss
    trains on; called once per keyframe, behind `lidar_depth_image`.  radius and tol have no default: they are the
    caller's policy, as admit_sweep's tolerances.  Returns a new image; want_counts adds an int32 device tensor
    {pixels kept, pixels removed}."""
    return _capi.lidar_occlusion_filter(lidar_depth.detach().contiguous(), radius, tol, want_counts)


class RobustLidarDepthLoss(torch.autograd.Function):
    """LidarDepthLoss with a Huber residual and a clip as one node (csrc/lidar.hip, gsr_lidar_depth_loss_robust): per
    candidate pixel tau = huber_abs + huber_rel z_L and clip = clip_abs + clip_rel z_L; |e| > clip is not supervised,
    |e| < tau is quadratic (0.5 e^2 / tau), the rest linear (|e| - tau / 2).  Gradients w.r.t. the rendered depth and
    silhouette only, scaled by the upstream scalar."""

    @staticmethod
    def forward(ctx, depth, acc, lidar_depth, acc_min, lambda_, huber_abs, huber_rel, clip_abs, clip_rel):
        need_d, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        out4, gd, ga = _capi.lidar_depth_loss_robust(depth.contiguous(), acc.contiguous(), lidar_depth.contiguous(),
                                                     acc_min, lambda_, huber_abs, huber_rel, clip_abs, clip_rel,
                                                     want_grad_depth=need_d, want_grad_acc=need_a)
        ctx.grads = (gd, ga)
        ctx.parts = out4  # [loss, mean |depth error| in metres, supervised share, clipped share] for logging
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        gd, ga = ctx.grads
        return ((gd * g if gd is not None else None), (ga * g if ga is not None else None)) + (None,) * 7


def lidar_depth_loss(depth, acc, lidar_depth, acc_min=0.5, lambda_=1.0, huber=0.0, huber_rel=0.0, clip=float("inf"),
                     clip_rel=0.0):
    """depth, acc: the second and third outputs of `render` ([H,W] or [1,H,W] f32 on the device, un-normalised);
    lidar_depth: `lidar_depth_image` of the same view (`lidar_occlusion_filter`ed or not).  acc_min = 0.5 is the
    threshold of the reference's silhouette masks (lioOptimization.cpp:1786-1792).  huber, huber_rel: the residual is
    quadratic below huber + huber_rel * z_L metres; clip, clip_rel: a pixel whose |depth error| exceeds
    clip + clip_rel * z_L is not supervised.  At their defaults (no quadratic zone, no clip) this is the plain masked
    L1 of `LidarDepthLoss`, the same node as ever; otherwise `RobustLidarDepthLoss`.  Returns the 0-dim loss."""
    if huber == 0.0 and huber_rel == 0.0 and clip == float("inf") and clip_rel == 0.0:
        return LidarDepthLoss.apply(depth, acc, lidar_depth, float(acc_min), float(lambda_))
    return RobustLidarDepthLoss.apply(depth, acc, lidar_depth, float(acc_min), float(lambda_), float(huber),
                                      float(huber_rel), float(clip), float(clip_rel))


def raster_K(width, height, FoVx, FoVy):
    """The intrinsics under which pixel (u, v) of a LiDAR depth image is pixel (u, v) of a render of the same camera:
    fx = W / (2 tan(FoVx / 2)), cx = (W - 1) / 2, likewise in y (the rasterizer's ndc2Pix puts the centre of pixel u at
    ((ndc + 1) W - 1) / 2).  [3,3] float64 on the host."""
    fx = width / (2.0 * math.tan(FoVx * 0.5))
    fy = height / (2.0 * math.tan(FoVy * 0.5))
    return torch.tensor([[fx, 0.0, (width - 1) * 0.5], [0.0, fy, (height - 1) * 0.5], [0.0, 0.0, 1.0]],
                        dtype=torch.float64)


def world_to_camera(camera):
    """[R | t] with x_c = R x_w + t, [3,4] float32 on the host, from the TRANSPOSED world-to-camera matrix a
    render_utils.Camera holds (world_view_transform, camera.cu:39-40)."""
    return camera.Get_world_view_transform().detach().cpu().t()[:3].contiguous().to(torch.float32)
