"""Reference of the camera-facing surfel normals (gsr_surfel_normals) and of the depth-normal consistency loss
(gsr_normal_consistency_loss): CPU, test infrastructure only.

Normals: numpy float64, straight from include/gsraster.h.  A row is FRAGILE, and left out of comparisons, when the facing
flip is decided by less than rounding distance, |n_c . p_c| <= 1e-4 |n_c| |p_c|, or when its two smallest scales differ
by less than 1e-6 relative WITHOUT being equal (an exact tie is decided by the lowest-index rule, which the tests
pin; the comparison of two given float32 values is exact in every implementation).  The fragile share is capped at
MAX_FRAGILE_SHARE; tests/test_normal_ref.py asserts it on the rows the GPU test uses.

Loss: `loss` is ONE composition of Torch ops, straight from the definitions; called on float64 tensors it is the
reference (gradients by autograd), called on float32 tensors it is the yardstick -- how far a float32 implementation is
from float64 before a different order of operations adds anything.  The yardstick adds its per-pixel rho in float64, as
the kernel does (sum_dtype); tools/time_normals.py times it with float32 sums.

Bars = 8 x the yardstick's worst error against float64 over the inputs of the tests (contrib_ref.B's convention; the
margin covers a different order of operations and summation tree), measured on the CPU -- tests/test_normal_ref.py
holds the reference to these figures:
  normals            |d| / |n_c|                      yardstick 1.4e-7   bar 1.12e-6
  out3               |d| / value                      yardstick 1.3e-7   bar 1.04e-6
  dL/ddepth, dL/dacc |d| / max |g64| over the image   yardstick 7.4e-6   bar 5.92e-5
(cases of `loss_case` at SHAPES, seeds 0..2, jump_rel +inf and 0.05, acc_min 0.5, normal_min 0.1, lambda 0.7: CASE_KW;
rows of `normal_rows`.)
"""
import math

import numpy as np
import torch

F32 = np.float32
MAX_FRAGILE_SHARE = 0.01
YARD_NORMALS, YARD_OUT3, YARD_GRADS = 1.4e-7, 1.3e-7, 7.4e-6
B_NORMALS, B_OUT3, B_GRADS = 8.0 * YARD_NORMALS, 8.0 * YARD_OUT3, 8.0 * YARD_GRADS

SHAPES = [(3, 3), (16, 17), (37, 23), (257, 3)]     # (W, H)
SEEDS = (0, 1, 2)
JUMPS = (float("inf"), 0.05)
CASE_KW = dict(acc_min=0.5, normal_min=0.1, lam=0.7)


# ---- normals ----------------------------------------------------------------------------------------------------------
def _columns(q, dt):
    w, x, y, z = (q[:, k].astype(dt) for k in range(4))
    one, two = dt(1), dt(2)
    c0 = np.stack([one - two * (y * y + z * z), two * (x * y + w * z), two * (x * z - w * y)], 1)
    c1 = np.stack([two * (x * y - w * z), one - two * (x * x + z * z), two * (y * z + w * x)], 1)
    c2 = np.stack([two * (x * z + w * y), two * (y * z - w * x), one - two * (x * x + y * y)], 1)
    return np.stack([c0, c1, c2], 1)    # [P, k, 3]: column k of R(q)


def surfel_normals(xyz, scaling, rotation, T_cw, dt=np.float64):
    """(normals [P,3], fragile [P] bool) in precision dt (float64: the reference; float32: the yardstick)"""
    xyz, scaling, rotation = (np.asarray(a, F32) for a in (xyz, scaling, rotation))
    T = np.asarray(T_cw, F32)[:3, :4].astype(dt)
    k = np.argmin(scaling, 1)                       # first occurrence of the minimum: the lowest index wins a tie
    n_w = _columns(rotation, dt)[np.arange(len(k)), k]
    n_c = n_w @ T[:, :3].T
    p_c = xyz.astype(dt) @ T[:, :3].T + T[:, 3]
    d = (n_c * p_c).sum(1)
    n = np.where((d > 0)[:, None], -n_c, n_c)
    s = np.sort(scaling.astype(np.float64), 1)
    near_tie = (s[:, 1] != s[:, 0]) & (np.abs(s[:, 1] - s[:, 0]) <= 1e-6 * np.abs(s[:, 1]))
    d64 = np.abs(d.astype(np.float64))
    fragile = (d64 <= 1e-4 * np.linalg.norm(n_c, axis=1) * np.linalg.norm(p_c, axis=1)) | near_tie
    return n.astype(dt), fragile


def normal_rows(P=300, seed=9):
    """rows for the GPU comparison: random centres in front of a camera, near-unit quaternions, scales with exact ties
    in every pattern, normals on both sides of the facing flip.  -> xyz, scaling, rotation (float32), T_cw [3,4]"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(-2, 2, (P, 2)), rng.uniform(1.0, 6.0, (P, 1))], 1).astype(F32)
    q = rng.normal(0, 1, (P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (P, 1))).astype(F32)
    s = rng.uniform(0.01, 0.3, (P, 3)).astype(F32)
    s[0:10, 1] = s[0:10, 0]; s[0:10, 2] = s[0:10, 0] * 2          # tie 0 = 1 < 2
    s[10:20, 2] = s[10:20, 1]; s[10:20, 0] = s[10:20, 1] * 2      # tie 1 = 2 < 0
    s[20:30, 2] = s[20:30, 0]; s[20:30, 1] = s[20:30, 0] * 2      # tie 0 = 2 < 1
    s[30:40, 1] = s[30:40, 0]; s[30:40, 2] = s[30:40, 0]          # all three equal
    a = math.radians(20.0)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    T = np.concatenate([R, np.array([[0.1], [-0.2], [0.3]])], 1).astype(F32)
    return xyz, s, q, T


# ---- the loss ------------------------------------------------------------------------------------------------------------
def loss(D, A, N, fx, fy, cx, cy, acc_min, normal_min, jump_rel, lam, sum_dtype=torch.float64):
    """-> (out3 [3] = {loss, mean rho, S / (W H)} in sum_dtype, S as an int, the supervised mask [H-2, W-2])
    D, A [H, W], N [3, H, W] of one dtype; differentiable towards D and A."""
    H, W = D.shape
    dt = D.dtype
    if H < 3 or W < 3:
        zero = (D.sum() + A.sum()) * 0.0
        return torch.stack([zero, zero, zero]).to(sum_dtype), 0, torch.zeros((max(H - 2, 0), max(W - 2, 0)), dtype=torch.bool)
    valid = A >= acc_min                                    # false for NaN
    z = torch.where(valid, D / torch.where(valid, A, torch.ones_like(A)), torch.zeros_like(D))
    u = torch.arange(W, dtype=dt)[None, :] - torch.tensor(cx, dtype=dt)
    v = torch.arange(H, dtype=dt)[:, None] - torch.tensor(cy, dtype=dt)
    X = torch.stack([u * z / torch.tensor(fx, dtype=dt), v * z / torch.tensor(fy, dtype=dt), z])
    c_, e_, w_, s_, n_ = (slice(1, -1), slice(1, -1)), (slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)), \
        (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))
    at = lambda t, sl: t[(Ellipsis,) + sl]                   # noqa: E731
    a = at(X, e_) - at(X, w_)
    b = at(X, s_) - at(X, n_)
    c = torch.stack([b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]])   # b x a
    clen = torch.sqrt((c * c).sum(0))
    Nc = at(N, c_)
    nlen = torch.sqrt((Nc * Nc).sum(0))
    with torch.no_grad():
        sup = at(valid, c_) & at(valid, e_) & at(valid, w_) & at(valid, s_) & at(valid, n_)
        zc = at(z, c_)
        if not math.isinf(jump_rel):
            lim = torch.tensor(jump_rel, dtype=dt) * zc
            for sl in (e_, w_, s_, n_):
                sup = sup & ((at(z, sl) - zc).abs() <= lim)
        sup = sup & (nlen >= torch.tensor(normal_min, dtype=dt) * at(A, c_)) & (clen > 0)
    one = torch.ones_like(clen)
    n_d = c / torch.where(sup, clen, one)
    n_r = Nc / torch.where(sup, nlen, one)
    rho = torch.where(sup, 1.0 - (n_r * n_d).sum(0), torch.zeros_like(clen))
    S = int(sup.sum())
    total = rho.to(sum_dtype).sum()
    mean = total / max(S, 1)
    out3 = torch.stack([lam * mean, mean, mean * 0.0 + S / float(W * H)])
    return out3, S, sup


def loss_and_grads(D, A, N, cam, acc_min, normal_min, jump_rel, lam, dt=torch.float64):
    """numpy in, numpy out: (out3 [3], dL/dD [H,W], dL/dA [H,W], S, supervised mask) in precision dt"""
    Dt = torch.tensor(np.asarray(D, F32), dtype=dt, requires_grad=True)
    At = torch.tensor(np.asarray(A, F32), dtype=dt, requires_grad=True)
    Nt = torch.tensor(np.asarray(N, F32), dtype=dt)
    out3, S, sup = loss(Dt, At, Nt, *[float(F32(v)) for v in cam], float(F32(acc_min)), float(F32(normal_min)),
                        float(F32(jump_rel)), float(F32(lam)))
    gd, ga = torch.autograd.grad(out3[0], (Dt, At), allow_unused=True)
    z = np.zeros(Dt.shape)
    return (out3.detach().double().numpy(), z if gd is None else gd.double().numpy(), z if ga is None else ga.double().numpy(),
            S, sup.numpy())


def camera(W, H, fov_deg=60.0):
    """(fx, fy, cx, cy) of raster_K for a square-pixel camera"""
    f = W / (2.0 * math.tan(math.radians(fov_deg) * 0.5))
    return f, f, (W - 1) * 0.5, (H - 1) * 0.5


def loss_case(W, H, seed=0):
    """A smooth random depth (three sinusoids on a ramp, z in [2, 6]), a silhouette in [0.6, 1] and random unit normals
    scaled by it.  -> D, A [H,W], N [3,H,W] float32, cam"""
    rng = np.random.default_rng(1000 * seed + 7 * W + H)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 4.0 + 0.6 * (u / max(W - 1, 1) - 0.5) + 0.4 * (v / max(H - 1, 1) - 0.5)
    for _ in range(3):
        k = rng.uniform(0.02, 0.25, 2)
        z = z + 0.4 * np.sin(k[0] * u + k[1] * v + rng.uniform(0, 2 * math.pi))
    assert z.min() >= 2.0 and z.max() <= 6.0
    A = rng.uniform(0.6, 1.0, (H, W))
    n = rng.normal(0, 1, (3, H, W))
    n /= np.linalg.norm(n, axis=0, keepdims=True)
    return (z * A).astype(F32), A.astype(F32), (n * A).astype(F32), camera(W, H)


def plane_case(W, H, normal=(0.3, -0.2, -1.0), dist=-4.0, theta=0.0):
    """The depth of the plane n . X = dist (n normalised, facing the camera: n_z < 0) under `camera(W, H)`, A = 1, and the
    normal image = n turned by theta about an axis perpendicular to it.  -> D, A, N (float64), cam, n"""
    cam = camera(W, H)
    fx, fy, cx, cy = cam
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)])
    z = dist / (n[:, None, None] * ray).sum(0)
    assert z.min() > 0
    t = np.cross(n, [0.0, 1.0, 0.0])
    t /= np.linalg.norm(t)
    nr = math.cos(theta) * n + math.sin(theta) * t
    return z, np.ones_like(z), np.broadcast_to(nr[:, None, None], (3, H, W)).copy(), cam, n


def rel(got, ref):
    """worst |got - ref| / |ref| over the elements with ref != 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = ref != 0
    return float((np.abs(got - ref)[m] / np.abs(ref)[m]).max(initial=0.0))


def grad_ratio(got, ref):
    """worst |got - ref| / max |ref| over the image"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = float(np.abs(ref).max(initial=0.0))
    return float(np.abs(got - ref).max(initial=0.0) / top) if top > 0 else float(np.abs(got).max(initial=0.0))
