"""Cameras whose two focal lengths differ, and scenes laid out in their frusta (test infrastructure).

Every other camera of the suite derives fovy = 2 atan(tan(fovx / 2) H / W): square pixels, for which the kernels'
focal_x = W / (2 tanfovx) and focal_y = H / (2 tanfovy) are the same float at almost every frame size, so a kernel that
reads one where it should read the other is bit-identical to the right one.  The reference takes its two fields of view
from two independently calibrated focal lengths (focal2fov(fx, cols), focal2fov(fy, rows)), and every camera it ships
has fx != fy (tests/golden/reference_intrinsics.json: name, width, height, fx, fy of its configuration files; the
principal point is never used -- its projection matrix is symmetric -- and is left out).

`camera` is poses.camera with the two fields of view from (fx, fy); `scene` fills that camera's anisotropic frustum with
make_gaussians' splats; INTRINSICS is the table of cases the CPU and GPU tests share.
"""
import functools
import json
import math
import os

import numpy as np

import poses as PZ
from gs_livm_amd import synthetic as S

BG = (0.2, 0.5, 0.9)


def focal2fov(focal, pixels):
    return 2.0 * math.atan(pixels / (2.0 * focal))


def camera(W, H, fx, fy, R_cw=None, T=None, dtype=np.float32):
    """poses.camera's arithmetic (hence make_camera's) with fovx = 2 atan(W / 2fx) and fovy = 2 atan(H / 2fy): R and T
    rounded to `dtype`, the translation row and view @ projection evaluated in `dtype`, the camera centre from the f64
    inverse of the view tensor, tanfovx / tanfovy rounded to f32 once."""
    fovx, fovy = focal2fov(fx, W), focal2fov(fy, H)
    R = np.asarray(np.eye(3) if R_cw is None else R_cw, np.float64).astype(dtype)
    T = np.asarray(np.zeros(3) if T is None else T, np.float64).astype(dtype)
    Tcw = np.eye(4, dtype=dtype)
    Tcw[:3, :3] = R.T
    Tcw[:3, 3] = -R.T @ T
    view = np.ascontiguousarray(Tcw.T)
    proj = np.ascontiguousarray(S.projection_matrix(S.ZNEAR, S.ZFAR, fovx, fovy).T).astype(dtype)
    full = (view @ proj).astype(dtype)
    campos = np.linalg.inv(view.astype(np.float64))[3, :3].astype(dtype)
    return {"W": int(W), "H": int(H), "tanfovx": float(np.float32(math.tan(fovx * 0.5))),
            "tanfovy": float(np.float32(math.tan(fovy * 0.5))), "viewmatrix": view, "projmatrix": full,
            "campos": campos}


def square_fx(W, fovx_deg=60.0):
    """The focal length of make_camera's square pixels."""
    return W / (2.0 * math.tan(math.radians(fovx_deg) / 2.0))


def scene(P, W, H, seed, D, fx, fy, pose=None):
    """make_scene with this camera: make_gaussians' splats over the camera's own frustum (horizontal field of view
    fovx, aspect of the two tangents (W / fx) / (H / fy)), optionally moved rigidly into the world with the camera by
    an entry of poses.POSES (means m R_cw^T + T in f64, rounded to f32 once, as poses.posed), background BG."""
    s = S.make_gaussians(P, seed, D, fovx_deg=math.degrees(focal2fov(fx, W)), aspect=(W / fx) / (H / fy))
    Rcw, T = (np.eye(3), np.zeros(3)) if pose is None else PZ.POSES[pose]
    if pose is not None:
        s["means3D"] = (s["means3D"].astype(np.float64) @ Rcw.T + T).astype(np.float32)
    s.update(camera(W, H, fx, fy, Rcw, T))
    s["bg"] = np.asarray(BG, np.float32)
    s["scale_modifier"] = 1.0
    s["colors_precomp"] = None
    s["cov3D_precomp"] = None
    return s


def reference_calibrations():
    """{name: dict(width, height, fx, fy)} of the reference's shipped configurations."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_intrinsics.json")
    with open(path) as f:
        return {e["name"]: e for e in json.load(f)}


def _ntu_quarter():
    c = reference_calibrations()["ntu"]
    assert c["width"] % 4 == 0 and c["height"] % 4 == 0
    return c["width"] // 4, c["height"] // 4, c["fx"] / 4.0, c["fy"] / 4.0


# name -> (W, H, fx, fy, pose of poses.POSES or None, (P, seed, SH degree)).  ntu/4 is the NTU calibration divided by
# four: a realistic 0.4 % between the two focal lengths.
INTRINSICS = {
    "ntu/4": _ntu_quarter() + (None, (1500, 13, 3)),
    "wide_y": (200, 120, 173.2, 104.0, None, (1500, 13, 3)),
    "tall_y": (200, 120, 120.0, 205.0, "rpy", (1500, 13, 3)),
    "tiny": (33, 17, 20.0, 31.0, "zup", (7, 3, 1)),
    "big": (257, 131, 260.0, 150.0, None, (2500, 5, 2)),
}
PATHS = ("jacobian_clamp", "cov3D_precomp", "scale_modifier")   # of helpers.REF64_PATHS, under wide_y's intrinsics


@functools.lru_cache(maxsize=None)
def entry(name):
    """(scene, seed) of one INTRINSICS entry; built once per process, not to be modified."""
    W, H, fx, fy, pose, (P, seed, D) = INTRINSICS[name]
    return scene(P, W, H, seed, D, fx, fy, pose), seed


@functools.lru_cache(maxsize=None)
def path_scene(kind):
    """(scene, seed) of one path of helpers.ref64_path_scene laid over wide_y's camera instead of make_scene's."""
    from helpers import ref64_path_scene
    W, H, fx, fy, pose, _ = INTRINSICS["wide_y"]

    def base(P, w, h, seed, D):
        assert (w, h) == (W, H)
        return scene(P, W, H, seed, D, fx, fy, pose)
    return ref64_path_scene(kind, base=base)


def with_fy_as_fx(sc):
    """The scene as a rasterizer that reads focal_x for focal_y would see it: tanfovy replaced by the f32 tangent for
    which H / (2 tanfovy) is W / (2 tanfovx).  (The Jacobian clamp's limit in y moves with it.)"""
    fx = np.float32(sc["W"]) / (np.float32(2.0) * np.float32(sc["tanfovx"]))
    return dict(sc, tanfovy=float(np.float32(sc["H"]) / (np.float32(2.0) * fx)))
