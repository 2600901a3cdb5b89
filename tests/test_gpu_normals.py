"""GPU tests of the camera-facing surfel normals (csrc/normal.hip k_surfel_normals through gsr_surfel_normals) and of the
rendered normal map (gs_livm_amd.render_normals = forward + normals + attribute blend).

Normals: against tests/normal_ref.py (numpy float64) off its fragile rows, |d| <= B_NORMALS |n_c| (8 x the float32
yardstick = 1.12e-6).
Normal map: a closed form that does not pass through the walk's reference -- coplanar surfels sharing one orientation
render, wherever anything was blended, a normal image parallel to the plane's normal.  Bar: every blended component
carries at most attr_ref.B sum w |n_k| <= attr_ref.B |N| of the walk and B_NORMALS of the normal itself, and the division
by |N| adds the relative error of the length (the same two terms): 2 (attr_ref.B + B_NORMALS) = 4.4e-5 per component."""
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G

import attr_ref as AR
import normal_ref as NR

pytestmark = pytest.mark.gpu


def test_normals_equal_float64_at_the_bar(gpu_device):
    xyz, s, q, T = NR.normal_rows()
    want, fragile = NR.surfel_normals(xyz, s, q, T)
    assert fragile.mean() <= NR.MAX_FRAGILE_SHARE
    dev = gpu_device
    out = torch.full((300 * 3 * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(300, 3)
    got = G._capi.surfel_normals(torch.from_numpy(xyz).to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(q).to(dev),
                                 torch.from_numpy(T), out=out).cpu().numpy()
    assert np.isfinite(got).all()                        # every row written
    d = np.abs(got.astype(np.float64) - want).max(1) / np.linalg.norm(want, axis=1)
    print("worst |d| / |n_c| %.3e (bar %.3e)" % (d[~fragile].max(), NR.B_NORMALS))
    assert (d[~fragile] <= NR.B_NORMALS).all()
    # the tie rows (0..39) are among them: the lowest index won
    assert not fragile[:40].any()
    # twice the same bits; the public wrapper is the same launch
    again = G.surfel_normals(torch.from_numpy(xyz).to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(q).to(dev),
                             torch.from_numpy(T))
    assert np.array_equal(again.cpu().numpy().view(np.int32), got.view(np.int32))


def test_a_normal_perpendicular_to_the_ray_is_not_flipped(gpu_device):
    dev = gpu_device
    xyz = torch.tensor([[0, 0, 3.0]] * 3, device=dev)
    q = torch.tensor([[1.0, 0, 0, 0]] * 3, device=dev)
    s = torch.tensor([[0.01, 0.2, 0.2], [0.2, 0.01, 0.2], [0.2, 0.2, 0.01]], device=dev)
    T = torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)
    n = G.surfel_normals(xyz, s, q, T).cpu().numpy()
    assert np.array_equal(n, np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32))   # n . p = 0 exactly: kept


class _Model:
    """the accessors render() asks a model for, over activated tensors"""

    def __init__(self, xyz, opacity, scaling, rotation, dev):
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
        self.xyz, self.opacity, self.scaling, self.rotation = f(xyz), f(opacity), f(scaling), f(rotation)
        self.features = torch.full((len(xyz), 1, 3), 0.5, device=dev)

    def Get_xyz(self): return self.xyz
    def Get_opacity(self): return self.opacity
    def Get_scaling(self): return self.scaling
    def Get_rotation(self): return self.rotation
    def Get_features(self): return self.features
    def Get_max_sh_degree(self): return 0


def _quat_z_to(n):
    """unit quaternion (w, x, y, z) turning the z axis onto the unit vector n"""
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(z, n)
    s, c = np.linalg.norm(axis), float(z @ n)
    half = 0.5 * math.atan2(s, c)
    return np.concatenate([[math.cos(half)], math.sin(half) * axis / s])


def test_coplanar_surfels_render_the_plane_normal(gpu_device):
    dev = gpu_device
    W, H, P = 70, 50, 200
    rng = np.random.default_rng(2)
    n = np.array([0.35, -0.25, 1.0])
    n /= np.linalg.norm(n)                              # the thin axis as stored: it faces AWAY from the camera
    xy = np.stack([rng.uniform(-1.5, 1.5, P), rng.uniform(-1.0, 1.0, P)], 1)
    z = 3.0 - (xy @ n[:2]) / n[2]                        # n . (x - (0, 0, 3)) = 0
    xyz = np.concatenate([xy, z[:, None]], 1)
    q = np.tile(_quat_z_to(n), (P, 1))
    scaling = np.tile([0.12, 0.12, 0.002], (P, 1))
    m = _Model(xyz, np.full((P, 1), 0.9), scaling, q, dev)
    fovx = math.radians(60.0)
    cam = G.Camera(np.eye(3), np.zeros(3), fovx, 2 * math.atan(math.tan(fovx / 2) * H / W), W, H, device=dev)
    color, depth, acc, radii, normals = G.render_normals(cam, m, torch.zeros(3, device=dev))
    assert normals.shape == (3, H, W) and color.shape == (3, H, W) and radii.shape == (P,)
    # the plane normal in camera axes (the camera sits at the origin, axes aligned), from the float32 quaternion the
    # kernel was given, turned towards the camera
    q32 = m.rotation[0].cpu().numpy()[None].astype(np.float32)
    want = -NR._columns(q32, np.float64)[0, 2]
    assert want[2] < 0 and abs(np.linalg.norm(want) - 1) < 1e-6 and np.abs(want + n).max() < 1e-6
    N = normals.cpu().numpy().astype(np.float64)
    on = acc[0].cpu().numpy() >= 0.5
    assert on.sum() > 500
    unit = N[:, on] / np.linalg.norm(N[:, on], axis=0)
    d = np.abs(unit - want[:, None] / np.linalg.norm(want)).max()
    bar = 2.0 * (AR.B + NR.B_NORMALS)
    print("worst |n_r - n| per component %.3e (bar %.3e) over %d pixels" % (d, bar, on.sum()))
    assert d <= bar
    # |N| = acc |n|: every blended normal is the same vector
    np.testing.assert_allclose(np.linalg.norm(N[:, on], axis=0), acc[0].cpu().numpy()[on] * np.linalg.norm(want), rtol=1e-4)
    # render_attributes is the same forward and walk
    at = G.surfel_normals(m.xyz, m.scaling, m.rotation, G.world_to_camera(cam))
    assert torch.equal(G.render_attributes(cam, m, torch.zeros(3, device=dev), at)[4].view(torch.int32),
                       normals.view(torch.int32))
    # and the loss takes the map as it comes (rho lies in [0, 2])
    K = G.raster_K(W, H, cam.Get_FoVx(), cam.Get_FoVy())
    loss = G.normal_consistency_loss(depth, acc, normals, K, 0.5, lambda_=1.0, normal_min=0.5, jump_rel=0.05)
    assert 0.0 <= float(loss) <= 2.0
