"""Host-side mirror of the two callers' views of the rasterizer that sit directly on top of the operator:

* `Camera`  -- the part of the reference's Camera the rasterizer consumes (include/gs/gs/camera.cuh:47-110,
  src/gs/camera.cu:14-57): world_view_transform (the transposed world-to-camera matrix), the projection of
  getProjectionMatrix (camera.cu:59-82, znear 0.01, zfar 100), full_proj_transform = view @ projection and the
  camera centre, with the reference's getter names.
* `render`  -- include/gs/gs/render_utils.cuh:13-56: settings from the camera, activated parameters from the model,
  one rasterizer call, (color, depth, depth_acc) back.  Differences, both in the caller's favour: no
  `torch.cuda.synchronize()` before the rasterizer (render_utils.cuh:49) and scalars stay on
  the host.  `override_color` is accepted as precomputed colours (the reference declares it and ignores it).
"""
import math

import torch

from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer

from .synthetic import ZFAR, ZNEAR, projection_matrix


def get_projection_matrix(znear, zfar, fov_x, fov_y):
    """getProjectionMatrix (src/gs/camera.cu:59-82) as the TENSOR the reference builds: Eigen stores P column-major and
    the reference wraps that memory as a row-major tensor, i.e. P transposed."""
    return torch.from_numpy(projection_matrix(znear, zfar, fov_x, fov_y).T.copy())


def se3_exp(xi):
    """Exp(xi^) of xi = (rho, phi) -- translation part first, rotation part second -- as a 4x4 transform
    [[R, V rho], [0, 1]], R = Exp(phi^), V the left Jacobian of SO(3).  Torch ops only, on xi's device and in its dtype,
    differentiable (at xi = 0 too), no host wait.  The coefficients are evaluated without cancellation: by their series
    below |phi| = 0.5, above it (1 - cos t) / t^2 as sin^2(t/2) / (t^2/2)."""
    if xi.shape != (6,):
        raise ValueError("se3_exp expects a tensor of shape (6,)")
    rho, phi = xi[:3], xi[3:]
    t2 = (phi * phi).sum()
    one = torch.ones_like(t2)
    big = t2 > 0.25
    t = torch.sqrt(torch.where(big, t2, one))             # only read where big: no sqrt at 0, whose derivative is not finite
    h = torch.sin(0.5 * t) / (0.5 * t)
    # below |phi| = 0.5 the three coefficients by their series in |phi|^2 (next term < 1e-16), analytic at 0
    sA = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0 + t2 * (
        -1.0 / 39916800.0 + t2 * (1.0 / 6227020800.0))))))
    sB = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0 + t2 * (
        -1.0 / 479001600.0 + t2 * (1.0 / 87178291200.0))))))
    sC = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (
        1.0 / 39916800.0 + t2 * (-1.0 / 6227020800.0)))))
    A = torch.where(big, torch.sin(t) / t, sA)
    B = torch.where(big, 0.5 * h * h, sB)
    Cc = torch.where(big, (t - torch.sin(t)) / (t * t * t), sC)
    z = torch.zeros_like(t)
    K = torch.stack([torch.stack([z, -phi[2], phi[1]]), torch.stack([phi[2], z, -phi[0]]),
                     torch.stack([-phi[1], phi[0], z])])
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    R = eye + A * K + B * K2
    V = eye + B * K + Cc * K2
    top = torch.cat([R, (V @ rho)[:, None]], 1)
    bottom = torch.cat([z.expand(3), one[None]])[None, :]
    return torch.cat([top, bottom], 0)


class Camera:
    """R: camera-to-world rotation [3,3], T: camera position [3] (the reference's _R, _T), FoVs in radians."""

    def __init__(self, R, T, FoVx, FoVy, image_width, image_height, device="cuda", uid=0, image_name=""):
        R = torch.as_tensor(R, dtype=torch.float32).cpu()
        T = torch.as_tensor(T, dtype=torch.float32).cpu()
        self._R, self._T, self._FoVx, self._FoVy = R, T, float(FoVx), float(FoVy)
        self._image_width, self._image_height = int(image_width), int(image_height)
        self._uid, self._image_name = uid, image_name
        Tcw = torch.eye(4, dtype=torch.float32)
        Tcw[:3, :3] = R.t()
        Tcw[:3, 3] = -(R.t() @ T)
        view = Tcw.t().contiguous()  # column-major Eigen memory read as a row-major tensor (camera.cu:39-40)
        proj = get_projection_matrix(ZNEAR, ZFAR, self._FoVx, self._FoVy)
        self._world_view_transform = view.to(device)
        self._projection_matrix = proj.to(device)
        self._full_proj_transform = (view @ proj).to(device)
        self._camera_center = torch.linalg.inv(view)[3, :3].contiguous().to(device)
        self._host_pose_stale = False

    def retract(self, xi):
        """T_cw <- Exp(xi^) T_cw (se3_exp; the left perturbation whose gradient render(..., pose_tangent=xi) leaves in
        xi.grad), then xi <- 0.  On the device, without a host wait, composed in float64 and rounded to float32 once;
        IN PLACE in the four device tensors: their addresses stay (the library keys a view's history by the view
        matrix's address).  Get_R / Get_T refresh their host copies on the next read (that read waits)."""
        with torch.no_grad():
            view = self._world_view_transform
            E = se3_exp(xi.detach().to(device=view.device, dtype=torch.float64))
            v64 = view.double() @ E.t()
            view.copy_(v64)
            self._full_proj_transform.copy_(v64 @ self._projection_matrix.double())
            self._camera_center.copy_(-(v64[:3, :3] @ v64[3, :3]))
            xi.zero_()
        self._host_pose_stale = True

    def _refresh_host_pose(self):
        if self._host_pose_stale:
            view = self._world_view_transform.detach().cpu()
            self._R = view[:3, :3].contiguous()           # view = T_cw^T: its upper block is the camera-to-world rotation
            self._T = -(view[:3, :3] @ view[3, :3])
            self._host_pose_stale = False

    def Get_image_height(self): return self._image_height
    def Get_image_width(self): return self._image_width
    def Get_FoVx(self): return self._FoVx
    def Get_FoVy(self): return self._FoVy
    def Get_uid(self): return self._uid
    def Get_image_name(self): return self._image_name
    def Get_R(self):
        self._refresh_host_pose()
        return self._R

    def Get_T(self):
        self._refresh_host_pose()
        return self._T

    def Get_world_view_transform(self): return self._world_view_transform
    def Get_projection_matrix(self): return self._projection_matrix
    def Get_full_proj_transform(self): return self._full_proj_transform
    def Get_camera_center(self): return self._camera_center


def render(viewpoint_camera, gaussian_model, bg_color, scaling_modifier=1.0, override_color=None, depth_gradient=False,
           pose_tangent=None):
    """-> (color [3,H,W], depth [1,H,W], depth_acc [1,H,W]); render_utils.cuh:13-56.
    depth_gradient=True (an extension): a loss on `depth` trains the Gaussians; by default its gradient stops at the
    rasterizer, as in the reference.
    pose_tangent (an extension): a zero [6] float32 leaf on the model's device; after loss.backward() its .grad holds
    the camera pose gradient dL/dxi of T_cw <- Exp(xi^) T_cw (several renders of one camera sum).  Step it with any
    optimiser, then viewpoint_camera.retract(pose_tangent) moves the camera and zeroes it again."""
    return render_full(viewpoint_camera, gaussian_model, bg_color, scaling_modifier, override_color, depth_gradient,
                       pose_tangent)[:3]


def render_full(viewpoint_camera, gaussian_model, bg_color, scaling_modifier=1.0, override_color=None,
                depth_gradient=False, pose_tangent=None):
    """`render` with the two outputs adaptive density control needs (upstream's render returns them too):
    -> (color, depth, depth_acc, radii [P] int32, means2D).  means2D is the [P,3] zero leaf whose .grad the backward
    fills with dL_dmean2D, unscaled: after loss.backward(), GrowableGaussians.accumulate_density(radii, means2D.grad)."""
    cam = viewpoint_camera
    dev = gaussian_model.Get_xyz().device
    settings = GaussianRasterizationSettings(
        image_height=int(cam.Get_image_height()), image_width=int(cam.Get_image_width()),
        tanfovx=math.tan(cam.Get_FoVx() * 0.5), tanfovy=math.tan(cam.Get_FoVy() * 0.5),
        bg=bg_color.to(dev), scale_modifier=float(scaling_modifier),
        viewmatrix=cam.Get_world_view_transform(), projmatrix=cam.Get_full_proj_transform(),
        sh_degree=int(gaussian_model.Get_max_sh_degree()), camera_center=cam.Get_camera_center(), prefiltered=False,
        depth_gradient=bool(depth_gradient))
    rasterizer = GaussianRasterizer(settings)
    if hasattr(gaussian_model, "activated"):  # one fused launch for all five getters
        means3D, opacity, scales, rotations, shs = gaussian_model.activated()
    else:
        means3D, opacity = gaussian_model.Get_xyz(), gaussian_model.Get_opacity()
        scales, rotations, shs = gaussian_model.Get_scaling(), gaussian_model.Get_rotation(), gaussian_model.Get_features()
    means2D = torch.zeros_like(means3D, requires_grad=True)
    if override_color is not None and override_color.numel():
        color, radii, depth, depth_acc = rasterizer(means3D, means2D, opacity, colors_precomp=override_color,
                                                    scales=scales, rotations=rotations, pose_tangent=pose_tangent)
    else:
        color, radii, depth, depth_acc = rasterizer(means3D, means2D, opacity, shs=shs, scales=scales,
                                                    rotations=rotations, pose_tangent=pose_tangent)
    return color, depth, depth_acc, radii, means2D
