"""LiDAR depth supervision (csrc/lidar.hip: gsr_lidar_depth_image, gsr_lidar_depth_loss) restated for the tests.

image64()     the z-buffer of a sweep: float64, a loop over the points with an explicit minimum.
image_ops()   the same in Torch ops (column arithmetic, scatter_reduce(amin)); dtype is a parameter: float64 must equal
              image64 exactly, float32 is the yardstick.
loss_ops()    the masked depth L1 in plain Torch with the gradients from autograd; float64 is the truth, float32 the
              yardstick.
bars()        the bound of the fused calls' error against float64 per compared quantity, and the fragile sets.
CASES / EXACT_CASES, inputs(), reference()   the inputs of tests/test_gpu_lidar.py and their references, evaluated
              once per process and not to be modified.

Bars.  eps = 2^-23 per counted rounding, as tests/delta_ref.py counts.  The kernel sees M = K [R | t] composed on the
host in double and rounded once; R and t themselves are float32 inputs and exact.  With hom = (|x|, |y|, |w|, 1),
N_abs = |M| hom and z_abs = |R_2| (|x|, |y|, |w|) + |t_z|:
  z = fma(r20, x, fma(r21, y, fma(r22, w, t_z)))         three fma                        dz = 4 eps z_abs    (3 counted)
  N_c = fma(m0, x, fma(m1, y, fma(m2, w, m3)))           four entry roundings, three fma  dN_c = 8 eps N_abs.c  (7 counted)
  X = N_x / N_z                                          one division
  X + 0.5                                                one addition
      dX = (dN_x + |X| dN_z) / |N_z| + eps |X| + eps (|X| + 0.5),   dY likewise
  lidar_depth[pixel] = min over its points: every candidate is off by at most its dz, so the minimum is off by at most
      the largest dz among the pixel's points; a pixel without a point is exactly 0 (bar 0: equality).
  e = D / A - z_L                  one division, one subtraction                          de = eps (|D / A| + |e|)
  mean|e|: f64 partial sums, one division, one narrowing; L one product more             dmean = sum de / n_sup + 3 eps mean,
                                                                                         dL = |lambda| dmean + eps |L|
  share = n_sup / (H W): exact count, one division, one narrowing                        2 eps share
  dL/dD = (c sign(e)) / A, c = lambda / n_sup narrowed once                               3 eps |dL/dD|   (2 counted)
  dL/dA = -(dL/dD) (D / A)                                                                5 eps |dL/dA|   (4 counted)
Every quantity is held to max(2 e_ref, its bar), e_ref = |float32 restatement - float64|.

Fragile items, removed from both sides (at most 1 % of a case's points and 1 % of its pixels, or the case fails):
  P1  a point whose X + 0.5 or Y + 0.5 lies within dX / dY of an integer (and that could land in or next to the image):
      it may fall into a neighbouring pixel; the up to four pixels it can reach are not compared
  P2  a point whose z lies within dz of min_depth or max_depth: kept or dropped; its pixel is not compared
      (the two counts are held to the number of fragile points / uncompared pixels)
  F3  a supervised pixel whose e lies within de of 0: the sign; removed from both gradients
  A and lidar_depth are inputs and compare with acc_min and 0 exactly on both sides -- their bar is 0 -- so no pixel is
  removed for them; the scenes hold pixels with A == acc_min exactly, which pins >= against >.
The EXACT_CASES (identity pose, power-of-two focal lengths, dyadic coordinates) have no rounding in any evaluation
order: they are compared bit for bit, without bars and without fragile sets, and they carry the points at exactly
min_depth, exactly max_depth, X = -0.5 (inside, pixel 0) and X = W - 0.5 (outside).
"""
import functools
import math

import numpy as np
import torch

import poses as PZ

F64 = torch.float64
EPS = 2.0 ** -23
COORD_MAX = 2.0 ** 30
MIN_DEPTH = float(np.float32(0.2))      # the rasterizer's near cull, as the kernel receives it
MAX_DEPTH = float(np.float32(10.0))
ACC_MIN = 0.5
LAMBDA = float(np.float32(0.7))


def _split(T_cw, K):
    T = np.asarray(T_cw, np.float64).reshape(-1, 4)[:3]
    return T[:, :3], T[:, 3], np.asarray(K, np.float64).reshape(3, 3)


def _tensor(a, dtype, device):
    return a.to(device=device, dtype=dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype, device=device)


def project64(points, T_cw, K):
    """Per point, float64, left to right: p = R x + t, N = K p, (X, Y) = N.xy / N.z; and the magnitudes bars() needs."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    R, t, K = _split(T_cw, K)
    with np.errstate(all="ignore"):
        p = [R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1] + R[r, 2] * x[:, 2] + t[r] for r in range(3)]
        N = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
        X, Y = N[0] / N[2], N[1] / N[2]
        M = np.abs(K @ np.concatenate([R, t[:, None]], 1))
        hom = np.concatenate([np.abs(x), np.ones((x.shape[0], 1))], 1)
        N_abs = hom @ M.T
        z_abs = np.abs(x) @ np.abs(R[2]) + abs(t[2])
    fin = np.isfinite(x).all(1) & np.isfinite(p[2]) & np.isfinite(X) & np.isfinite(Y)
    return dict(x=x, z=p[2], X=X, Y=Y, Nz=N[2], N_abs=N_abs, z_abs=z_abs, finite=fin)


def image64(points, T_cw, K, H, W, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """(image [H,W] float64, points kept, pixels hit, project64's dict): the contract of gsr_lidar_depth_image."""
    e = project64(points, T_cw, K)
    img = np.zeros((H, W), np.float64)
    seen = np.zeros((H, W), bool)
    kept = 0
    for i in range(e["x"].shape[0]):
        if not e["finite"][i]:
            continue
        z, X, Y = float(e["z"][i]), float(e["X"][i]), float(e["Y"][i])
        if z <= min_depth or z > max_depth:
            continue
        if abs(X) > COORD_MAX or abs(Y) > COORD_MAX:
            continue
        ix, iy = math.floor(X + 0.5), math.floor(Y + 0.5)
        if ix < 0 or ix >= W or iy < 0 or iy >= H:
            continue
        kept += 1
        if not seen[iy, ix] or z < img[iy, ix]:
            img[iy, ix] = z
            seen[iy, ix] = True
    return img, kept, int(seen.sum()), e


def image_ops(points, T_cw, K, H, W, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, dtype=F64, device="cpu", counts=True):
    """(image [H,W], points kept, pixels hit) in Torch ops of one dtype: what a caller composes without the fused call
    (tools/time_lidar_depth.py times it, with counts=False: the image alone, no read-back)."""
    x = _tensor(points, dtype, device).reshape(-1, 3)
    T, K = _tensor(T_cw, dtype, device).reshape(-1, 4)[:3], _tensor(K, dtype, device).reshape(3, 3)
    R, t = T[:, :3], T[:, 3]
    p = [R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1] + R[r, 2] * x[:, 2] + t[r] for r in range(3)]
    N = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
    X, Y, z = N[0] / N[2], N[1] / N[2], p[2]
    ok = torch.isfinite(x).all(1) & torch.isfinite(z) & torch.isfinite(X) & torch.isfinite(Y)
    ok = ok & (z > min_depth) & (z <= max_depth) & (X.abs() <= COORD_MAX) & (Y.abs() <= COORD_MAX)
    ix = torch.floor(torch.where(ok, X, torch.zeros_like(X)) + 0.5).long()
    iy = torch.floor(torch.where(ok, Y, torch.zeros_like(Y)) + 0.5).long()
    ok = ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    # (a dropped point goes to a spare slot behind the image: no boolean indexing, hence no host synchronisation)
    idx = torch.where(ok, iy * W + ix, torch.full_like(ix, H * W))
    img = torch.full((H * W + 1,), float("inf"), dtype=dtype, device=device)
    img = img.scatter_reduce(0, idx, z, "amin", include_self=True)[:H * W]
    hit = torch.isfinite(img)
    img = torch.where(hit, img, torch.zeros_like(img))
    if not counts:
        return img.reshape(H, W)
    return img.reshape(H, W), int(ok.sum()), int(hit.sum())


def loss_forward_ops(D, A, zl, acc_min, lam):
    """(loss, mean |e|, supervised share) on tensors of one dtype and shape; differentiable in D and A."""
    sup = (zl > 0) & (A >= acc_min)
    safe = torch.where(sup, A, torch.ones_like(A))
    e = torch.where(sup, D / safe - zl, torch.zeros_like(D))
    n = sup.sum()
    mean = e.abs().sum() / n.clamp_min(1).to(D.dtype)
    return lam * mean, mean, n.to(D.dtype) / D.numel()


def loss_ops(depth, acc, lidar, acc_min=ACC_MIN, lam=LAMBDA, dtype=F64):
    """{loss, mean, share, grad_depth, grad_acc} of the masked depth L1, gradients from autograd."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    D, A, zl = t(depth).clone().requires_grad_(True), t(acc).clone().requires_grad_(True), t(lidar)
    loss, mean, share = loss_forward_ops(D, A, zl, acc_min, lam)
    gD, gA = torch.autograd.grad(loss, [D, A], allow_unused=True)
    z = lambda g: (torch.zeros_like(D) if g is None else g).detach()  # noqa: E731
    return dict(loss=loss.detach(), mean=mean.detach(), share=share.detach(), grad_depth=z(gD), grad_acc=z(gA))


def bars(e, H=None, W=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """Bars and fragile sets (module docstring).  e: project64's dict (with H, W: the image) or the float64 loss_ops
    dict extended by its inputs (depth, acc, lidar, acc_min, lam)."""
    if "X" in e:
        with np.errstate(all="ignore"):
            X, Y, Nz = np.abs(e["X"]), np.abs(e["Y"]), np.abs(e["Nz"])
            dN = 8 * EPS * e["N_abs"]
            dX = (dN[:, 0] + X * dN[:, 2]) / Nz + EPS * X + EPS * (X + 0.5)
            dY = (dN[:, 1] + Y * dN[:, 2]) / Nz + EPS * Y + EPS * (Y + 0.5)
            dz = 4 * EPS * e["z_abs"]
            fr = lambda v: np.abs(v - np.round(v))  # noqa: E731
            fin = e["finite"]
            near = fin & (e["X"] > -1.5 - dX) & (e["X"] < W + 0.5 + dX) & (e["Y"] > -1.5 - dY) & (e["Y"] < H + 0.5 + dY)
            live = near & (e["z"] > min_depth - dz) & (e["z"] <= max_depth + dz)
            P1 = live & ((fr(e["X"] + 0.5) <= dX) | (fr(e["Y"] + 0.5) <= dY))
            P2 = near & ((np.abs(e["z"] - min_depth) <= dz) | (np.abs(e["z"] - max_depth) <= dz))
        keep = np.ones((H, W), bool)
        for i in np.nonzero(P1 | P2)[0]:
            for sx in (-dX[i], dX[i]):
                for sy in (-dY[i], dY[i]):
                    ix, iy = math.floor(e["X"][i] + 0.5 + sx), math.floor(e["Y"][i] + 0.5 + sy)
                    if 0 <= ix < W and 0 <= iy < H:
                        keep[iy, ix] = False
        bar = np.zeros((H, W), np.float64)
        ok = fin & ~(P1 | P2) & (e["z"] > min_depth) & (e["z"] <= max_depth) & (X <= COORD_MAX) & (Y <= COORD_MAX)
        ix = np.floor(np.where(ok, e["X"], 0.0) + 0.5).astype(np.int64)
        iy = np.floor(np.where(ok, e["Y"], 0.0) + 0.5).astype(np.int64)
        ok &= (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        np.maximum.at(bar, (iy[ok], ix[ok]), dz[ok])
        return dict(bar=bar, keep=keep, P1=P1, P2=P2, dX=dX, dY=dY, dz=dz)
    D, A, zl = (torch.as_tensor(np.asarray(e[k]), dtype=F64) for k in ("depth", "acc", "lidar"))
    sup = (zl > 0) & (A >= e["acc_min"])
    q = torch.where(sup, D / torch.where(sup, A, torch.ones_like(A)), torch.zeros_like(D))
    err = torch.where(sup, q - zl, torch.zeros_like(D))
    de = torch.where(sup, EPS * (q.abs() + err.abs()), torch.zeros_like(D))
    n = max(int(sup.sum()), 1)
    dmean = float(de.sum()) / n + 3 * EPS * float(e["mean"])
    lam = abs(float(e["lam"]))
    return dict(bar=dict(mean=dmean, loss=lam * dmean + EPS * abs(float(e["loss"])), share=2 * EPS * float(e["share"]),
                         grad_depth=3 * EPS * e["grad_depth"].abs(), grad_acc=5 * EPS * e["grad_acc"].abs()),
                F3=sup & (err.abs() <= de), sup=sup, e=err, de=de)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------
# name -> (R_cw, T): camera-to-world rotation and camera position, float64 (tests/poses.py's conventions)
POSES = {
    "identity": (np.eye(3), np.zeros(3)),
    "yaw": (PZ.rotation(yaw=25.0), np.array([0.3, 0.0, -0.2])),
    "rpy": PZ.POSES["rpy"],                 # every entry of R non-zero: a transposed R is another matrix
}
# (name, H, W, n, pose, seed): the smallest shapes at which the kernels can go wrong -- one pixel, an odd sliver, seams
# on both axes, exactly 20 workgroups, and 512 x 640 once (1280 partial sums: the finish walks more than 256); n on
# both sides of a workgroup of points, none at all, and more points than pixels (several per pixel)
CASES = (("1x1_n1", 1, 1, 1, "identity", 1), ("3x5_n0", 3, 5, 0, "yaw", 2), ("3x5_n255", 3, 5, 255, "rpy", 3),
         ("37x61_n256", 37, 61, 256, "identity", 4), ("37x61_n257", 37, 61, 257, "rpy", 5),
         ("64x80_n5000", 64, 80, 5000, "yaw", 6), ("70x130_n5000", 70, 130, 5000, "rpy", 7),
         ("70x130_n70001", 70, 130, 70001, "yaw", 8), ("512x640_n70001", 512, 640, 70001, "rpy", 9))
CASE_NAMES = tuple(c[0] for c in CASES)
EXACT_CASES = (("exact_3x5", 3, 5, 257, 21), ("exact_37x61", 37, 61, 5000, 22))
EXACT_NAMES = tuple(c[0] for c in EXACT_CASES)
EXACT_K = np.array([[4.0, 0.0, 2.0], [0.0, 8.0, 1.0], [0.0, 0.0, 1.0]], np.float32)   # powers of two, fx != fy, off centre
EXACT_MIN, EXACT_MAX = 0.25, 8.0
EXACT_T = np.eye(4, dtype=np.float32)[:3]


def intrinsics(H, W):
    """K with fx != fy and the principal point off the centre ((W - 1) / 2, (H - 1) / 2), float32."""
    return np.array([[0.9 * W, 0, (W - 1) / 2 + 1.3], [0, 1.07 * W, (H - 1) / 2 - 0.7], [0, 0, 1]], np.float32)


def pose(name):
    """T_cw = [R_cw^T | -R_cw^T T], [3,4] float32 (computed in float64, rounded once)."""
    R_cw, T = POSES[name]
    return np.concatenate([R_cw.T, (-R_cw.T @ T)[:, None]], 1).astype(np.float32)


def _exact_points(H, W, n, seed):
    """Dyadic points in the camera frame (= the world: identity pose) whose X, Y and z are exact in float32 in any
    evaluation order.  Random ones over rows < H - 2 (X and Y on a grid of quarter pixels from -1 to past the far
    edges, z a power of two from min_depth to twice max_depth), and in the last two rows, each alone in its pixel:
    z == min_depth (dropped), z == max_depth (kept), z == 2 max_depth (dropped), X = -0.5 (pixel 0), X = W - 0.5
    (outside)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = EXACT_K[0, 0], EXACT_K[1, 1], EXACT_K[0, 2], EXACT_K[1, 2]
    X = rng.integers(-4, 4 * W + 2, n) / 4.0
    Y = rng.integers(-4, 4 * (H - 2) - 2, n) / 4.0                 # Y + 0.5 < H - 2: rows 0 .. H - 3
    z = 2.0 ** rng.integers(-2, 5, n)                              # 0.25 .. 16
    special = [(0.0, H - 1.0, EXACT_MIN), (2.0, H - 1.0, EXACT_MAX), (4.0, H - 1.0, 2 * EXACT_MAX),
               (-0.5, H - 2.0, 2.0), (W - 0.5, H - 2.0, 2.0), (3.25, H - 2.0, -1.0)]
    k = len(special)
    for j, (sx, sy, sz) in enumerate(special):
        X[n - k + j], Y[n - k + j], z[n - k + j] = sx, sy, sz
    pts = np.stack([(X - cx) / fx * z, (Y - cy) / fy * z, z], 1)
    assert (pts.astype(np.float32).astype(np.float64) == pts).all()
    return pts.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The float32 inputs of one of CASES or EXACT_CASES.
    Sweep: points laid out in the camera frame -- pixel coordinates from 15 % outside the image on every side, z from
    0.5 m to 12 m (max_depth is 10), one in sixteen behind the camera -- and moved into the world with the camera; from
    eight points on, one NaN and one Inf coordinate.
    Render: A in [0.3, 1] (both sides of acc_min) with a few pixels at exactly acc_min; D = A (z_L + an offset of up to
    +-0.4 m), over the holes of the LiDAR image A (5 m + offset); from 1000 pixels on, two pixels with e == 0 exactly."""
    for name, H, W, n, seed in EXACT_CASES:
        if name == case:
            return dict(points=_exact_points(H, W, n, seed), T_cw=EXACT_T, K=EXACT_K, H=H, W=W, n=n,
                        min_depth=EXACT_MIN, max_depth=EXACT_MAX, exact=True)
    name, H, W, n, pname, seed = next(c for c in CASES if c[0] == case)
    rng = np.random.default_rng(seed)
    K, T_cw = intrinsics(H, W), pose(pname)
    R_cw, T = POSES[pname]
    K64 = K.astype(np.float64)
    if n == 1:
        u, v = np.array([0.1]), np.array([-0.2])
    else:
        u = rng.uniform(-0.15 * W - 0.5, 1.15 * W - 0.5, n)
        v = rng.uniform(-0.15 * H - 0.5, 1.15 * H - 0.5, n)
    z = rng.uniform(0.5, 12.0, n)
    behind = rng.uniform(0, 1, n) < 1.0 / 16.0
    z = np.where(behind & (n > 1), -rng.uniform(0.3, 5.0, n), z)
    cam = np.stack([(u - K64[0, 2]) / K64[0, 0] * z, (v - K64[1, 2]) / K64[1, 1] * z, z], 1)
    pts = (cam @ R_cw.T + T).astype(np.float32).reshape(n, 3)
    if n >= 8:
        pts[3, 0] = np.nan
        pts[5, 2] = np.inf
    zl = image64(pts, T_cw, K, H, W)[0].astype(np.float32)
    A = rng.uniform(0.3, 1.0, (H, W))
    off = rng.uniform(0.05, 0.4, (H, W)) * (rng.integers(0, 2, (H, W)) * 2 - 1)
    D = A * (np.where(zl > 0, zl, 5.0) + off)
    A, D = A.astype(np.float32), D.astype(np.float32)
    if H * W >= 15:
        A.reshape(-1)[::7][:5] = np.float32(ACC_MIN)                 # A == acc_min exactly: supervised (>=)
    if H * W >= 1000:
        hit = np.nonzero(zl.reshape(-1) > 0)[0]
        for j in hit[[len(hit) // 3, 2 * len(hit) // 3]]:
            A.reshape(-1)[j] = 1.0
            D.reshape(-1)[j] = zl.reshape(-1)[j]                     # D / 1 - z_L == 0 exactly: sign(0) = 0
    return dict(points=pts, T_cw=T_cw, K=K, H=H, W=W, n=n, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, exact=False,
                depth=D, acc=A, lidar=zl, acc_min=ACC_MIN, lam=LAMBDA)


def _image_args(x):
    return (x["points"], x["T_cw"], x["K"], x["H"], x["W"], x["min_depth"], x["max_depth"])


@functools.lru_cache(maxsize=None)
def reference(case):
    """Image: float64 truth, float32 yardstick, final bars, the pixels compared and the fragile counts.  Loss (CASES
    only): the same.  Exact cases: the image and the counts, to be met bit for bit."""
    x = inputs(case)
    H, W = x["H"], x["W"]
    img, kept, hit, e = image64(*_image_args(x))
    if x["exact"]:
        assert (img.astype(np.float32).astype(np.float64) == img).all()
        return dict(image=img, kept=kept, hit=hit, proj=e)
    img32, kept32, hit32 = image_ops(*_image_args(x), dtype=torch.float32)
    b = bars(e, H, W, x["min_depth"], x["max_depth"])
    eref = np.abs(img32.numpy().astype(np.float64) - img)
    n_frag = int((b["P1"] | b["P2"]).sum())
    image = dict(truth=img, kept=kept, hit=hit, f32=img32.numpy(), kept32=kept32, hit32=hit32,
                 bar=np.maximum(2 * eref, b["bar"]), keep=b["keep"], fragile_points=n_frag,
                 fragile_pixels=int((~b["keep"]).sum()), eref=eref)
    t = loss_ops(x["depth"], x["acc"], x["lidar"], x["acc_min"], x["lam"])
    y32 = loss_ops(x["depth"], x["acc"], x["lidar"], x["acc_min"], x["lam"], dtype=torch.float32)
    lb = bars(dict(t, depth=x["depth"], acc=x["acc"], lidar=x["lidar"], acc_min=x["acc_min"], lam=x["lam"]))
    bar, er = {}, {}
    for k in ("loss", "mean", "share", "grad_depth", "grad_acc"):
        er[k] = (y32[k].to(F64) - t[k]).abs()
        bar[k] = torch.maximum(2 * er[k], torch.as_tensor(lb["bar"][k], dtype=F64))
    loss = dict(truth=t, f32=y32, bar=bar, keep=~lb["F3"], fragile_pixels=int(lb["F3"].sum()), eref=er,
                n_sup=int(lb["sup"].sum()))
    return dict(image=image, loss=loss)


def fragile_shares(ref, x):
    """(share of fragile points, share of uncompared image pixels, share of fragile loss pixels) of one case."""
    n, N = max(x["n"], 1), x["H"] * x["W"]
    return (ref["image"]["fragile_points"] / n, ref["image"]["fragile_pixels"] / N, ref["loss"]["fragile_pixels"] / N)


def _ratio(d, bar, keep):
    d, bar = np.asarray(d, np.float64), np.asarray(bar, np.float64)
    r = np.where(bar > 0, d / np.maximum(bar, 1e-300), np.where(d == 0, 0.0, 1e9))   # a bar of 0 demands equality
    return float(np.where(keep, r, 0.0).max(initial=0.0))


def image_ratios(got, kept, hit, ref):
    """worst |got - truth| / bar over the compared pixels, and the two counts against their slack (fragile points /
    uncompared pixels); got: [H,W] array."""
    im = ref["image"]
    d = np.abs(np.asarray(got, np.float64) - im["truth"])
    d = np.where(np.isfinite(d), d, 1e30)
    cnt = lambda g, t, slack: 0.0 if g == t else (abs(g - t) / slack if slack else 1e9)  # noqa: E731
    return dict(image=_ratio(d, im["bar"], im["keep"]), kept=cnt(kept, im["kept"], im["fragile_points"]),
                hit=cnt(hit, im["hit"], im["fragile_pixels"]))


def loss_ratios(got, ref):
    """worst |got - truth| / bar per quantity; got: {loss, mean, share: float, grad_depth, grad_acc: float64 tensor}."""
    lo = ref["loss"]
    out = {}
    for k in ("grad_depth", "grad_acc"):
        d = (got[k].to(F64).reshape(lo["truth"][k].shape) - lo["truth"][k]).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, 1e30))
        out[k] = _ratio(d.numpy(), lo["bar"][k].numpy(), lo["keep"].numpy())
    for k in ("loss", "mean", "share"):
        out[k] = _ratio(abs(float(got[k]) - float(lo["truth"][k])), float(lo["bar"][k]), True)
    return out
