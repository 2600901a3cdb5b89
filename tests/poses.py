"""Posed scenes: the known test scenes seen by cameras with roll, pitch and translation (test infrastructure).

Every camera of gs_livm_amd.synthetic.make_camera is a yaw about +y, for which the world-to-camera rotation has
R[0][1] = R[1][0] = R[1][2] = R[2][1] = 0: in the row-major tensor the kernels index, viewmatrix[1], [4], [6] and [9]
are exactly 0.0, and a kernel that reads the matrix transposed in those places is bit-identical to the right one.
`posed` moves a scene rigidly into the world together with its camera, so the frame stays the known one (same splats
in the same part of the image) while the view matrix becomes dense.

Conventions: R_cw is the camera-to-world rotation (columns = the camera's right, down and forward axes in the world),
T the camera position, both float64.  The camera looks down its +z, x to the right, y down (src/gs/camera.cu:36-48).
"""
import math

import numpy as np

from gs_livm_amd import synthetic as S


def _cs(deg):
    """(cos, sin) of an angle in degrees, exact at multiples of 90."""
    q, r = divmod(float(deg), 90.0)
    if r == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    a = math.radians(deg)
    return math.cos(a), math.sin(a)


def rotation(roll=0.0, pitch=0.0, yaw=0.0):
    """R_cw = Ry(yaw) Rx(pitch) Rz(roll), degrees, float64: roll about the optical axis, pitch about the camera's x,
    yaw about +y as make_camera's."""
    (cr, sr), (cp, sp), (cy, sy) = _cs(roll), _cs(pitch), _cs(yaw)
    Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    return Ry @ Rx @ Rz


# optical axis along world +x, image right = world -y, image down = world -z: a LiDAR-inertial body frame, z up
ZUP = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
RPY = rotation(roll=37.0, pitch=-22.0, yaw=140.0)
ZUP_TILTED = ZUP @ rotation(roll=4.0, pitch=-3.0, yaw=5.0)

# Direction of the translations of the reach-of-float32 table (tests/test_poses.py) and the
# largest distance along it at which the f32 oracle alone stays at <= 0.5 of every f64 bar under ZUP_TILTED.
REACH_DIR = np.array([35.0, -12.0, 4.0]) / math.sqrt(35.0 ** 2 + 12.0 ** 2 + 4.0 ** 2)
REACH_DISTANCES = (0.0, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0)
REACH = 10.0

# name -> (R_cw, T).  PURE poses turn about one camera axis only (some of viewmatrix[1], [4], [6], [9] stay zero).
POSES = {
    "roll90": (rotation(roll=90.0), np.zeros(3)),
    "pitch+35": (rotation(pitch=35.0), np.array([1.5, -0.5, 2.0])),
    "pitch-35": (rotation(pitch=-35.0), np.zeros(3)),
    "rpy": (RPY, np.array([-1.5, 2.0, 2.5])),
    "zup": (ZUP_TILTED, REACH * REACH_DIR),
    "behind": (rotation(yaw=180.0), np.array([-2.0, 0.5, 4.0])),
    "far": (ZUP_TILTED, np.array([310.0, -140.0, 22.0])),
}
PURE = ("roll90", "pitch+35", "pitch-35", "behind")
WITHIN_REACH = tuple(k for k in POSES if k != "far")     # the poses compared with f64 at the fixed bars


def camera(W, H, R_cw, T, fovx_deg=60.0, dtype=np.float32):
    """make_camera's arithmetic (gs_livm_amd/synthetic.py) from a general R_cw and T: R and T rounded to `dtype`, the
    translation row -R^T T and view @ projection evaluated in `dtype`, the camera centre from the f64 inverse of the
    view tensor.  With dtype=np.float64 nothing is rounded (the rigid-invariance check of ref64 needs that)."""
    fovx = math.radians(fovx_deg)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    R = np.asarray(R_cw, np.float64).astype(dtype)
    T = np.asarray(T, np.float64).astype(dtype)
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


def posed(scene, R_cw, T, fovx_deg=60.0):
    """The scene (S.make_scene / helpers.ref64_path_scene: Gaussians laid out in the frustum of the origin camera)
    moved rigidly into the world with its camera: means m R_cw^T + T evaluated in f64 and rounded to f32 once,
    viewmatrix / projmatrix / campos rebuilt as make_camera builds them.  Everything else is shared with `scene`
    (a world-frame cov3D_precomp is not turned: take it from the oracle frame of the POSED scene, posed_path_scene)."""
    R_cw, T = np.asarray(R_cw, np.float64), np.asarray(T, np.float64)
    sc = dict(scene)
    cam = camera(scene["W"], scene["H"], R_cw, T, fovx_deg)
    assert cam["tanfovx"] == scene["tanfovx"] and cam["tanfovy"] == scene["tanfovy"], "posed(): another field of view"
    sc.update(cam)
    sc["means3D"] = (np.asarray(scene["means3D"], np.float64) @ R_cw.T + T).astype(np.float32)
    return sc


def posed_path_scene(kind, R_cw, T):
    """(scene, seed) of one path of helpers.REF64_PATHS under a pose; the precomputed covariance is the oracle's own
    of the posed scene (world frame: only the view matrix turns it into the camera frame)."""
    from helpers import ref64_path_scene
    if kind != "cov3D_precomp":
        sc, seed = ref64_path_scene(kind)
        return posed(sc, R_cw, T), seed
    from oracle import oracle as O
    sc = posed(S.make_scene(1500, 200, 120, 13, sh_degree=1), R_cw, T)
    base = O.forward(sc, keep_handle=False)
    cov = base.cov3D.copy()
    cov[base.radii <= 0] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32)
    sc["cov3D_precomp"] = cov
    sc["scales"] = None
    sc["rotations"] = None
    return sc, 13


def quat_of(R):
    """Unit quaternion (r, x, y, z) of a rotation matrix, f64 (Shepperd's branches)."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = np.array([tr, R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(cand))
    if k == 0:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2.0 * R[0, 0] - tr, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2.0 * R[1, 1] - tr, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2.0 * R[2, 2] - tr])
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    """Hamilton product a (4,) x b (n, 4), (r, x, y, z)."""
    ar, ax, ay, az = a
    br, bx, by, bz = np.asarray(b, np.float64).T
    return np.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                     ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], 1)


def ratios_against_ref64(fr, r, g):
    """{image or gradient group: worst |d| / bar} of an f32 frame (fr's images, gradients g) against
    r = ref64.render(..., slack=True).  The bars are those of helpers.check_against_ref64, which asserts them; this
    only measures, so that a table can go past 1."""
    ok = fr.fragile == 0
    out = {}
    for name in ("out_color", "out_depth", "out_acc"):
        ref = r[name]
        scale = max(1.0, float(np.abs(ref).max())) if name == "out_depth" else 1.0
        err = np.abs(np.asarray(getattr(fr, name), np.float64).reshape(ref.shape) - ref).max(0)
        out[name] = float(err[ok].max(initial=0)) / (1e-4 * scale)
    for k, got in g.items():
        ref = r[k].reshape(np.shape(got))
        if ref.size == 0:
            continue
        P = ref.shape[0]
        shape = (P,) + (1,) * (ref.ndim - 1)
        tol = 1e-5 * float(np.abs(ref).max()) + 1e-4 * np.abs(ref.reshape(P, -1)).max(1).reshape(shape)
        tol = tol + r["slack"][k].reshape(P, -1).max(1).reshape(shape)
        out[k] = float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())
    return out
