"""Sweep admission (csrc/seed.hip: gsr_sweep_admit) restated for the tests, from the rules of include/gsraster.h.

admit64()     float64, a loop over the points with explicit minima and an explicit winner per pixel.
admit_ops()   the same in Torch ops (what a host composes without the fused call: column arithmetic, a pooled window
              minimum, two scatter_reduce(amin), a nonzero and the gathers); dtype is a parameter: float64 must equal
              admit64 exactly, float32 is the yardstick and what tools/time_sweep_admit.py times.
bars()        the bound of the fused call's error against float64 per continuous output, and the fragile points.
CASES / EXACT_CASES, inputs(), reference()   the inputs of tests/test_gpu_seed.py and their references, evaluated once
              per process and not to be modified.
hole_scene()  the end-to-end scene: a surface of 600 Gaussians at 70 x 50 with the rows of one image region removed.

Bars.  eps = 2^-23 per counted rounding, as tests/lidar_ref.py counts; z, X, Y and their bars dz, dX, dY are
lidar_ref.bars' (the projection is the same code).  depth, acc, lidar_depth, image, exposure and covs are float32
inputs and exact; the tolerances and the footprint are passed as float32 values.
  z_out = z                                                                               dz
  sigma^2:  f z (1 rounding), times 2 (exact), fx + fy (1), the division (1), the square (1): four roundings, the
      first three doubled by the square, and z's own error twice                         var (2 dz / z + 8 eps)
  colour, per channel, V = the largest |tap|:
      tx = X - floor(X), ty likewise: one rounding each, each moving the sample by at most eps times a tap difference
          (<= 2 V)                                                                        4 eps V
      three lerps a + t (b - a): three roundings each on magnitudes <= 2 V, 2 V and V: 5 eps V; the vertical lerp
          carries the horizontal ones' error with weights that sum to one                 10 eps V
      the sample's sensitivity to the projection, from the four taps:
          |dv/dX| = |(1 - ty)(v01 - v00) + ty (v11 - v10)|, |dv/dY| = |bot - top|         |dv/dX| dX + |dv/dY| dY
      dv = 14 eps V + |dv/dX| dX + |dv/dY| dY
      u = (v - b) / g: one subtraction, one division                                      du = dv / |g| + 2 eps |u|
      c = 255 u: one product                                                              dc = 255 du + eps |c|
Every continuous output is held to max(2 e_ref, its bar), e_ref = |float32 restatement - float64|.

Fragile points, removed from both sides (at most 1 % of a case's points, or the case fails):
  P1, P2  of lidar_ref.bars: the pixel, or min_depth / max_depth, within the projection's bar
  T2  z - zmin within  dz (1 + tol) + eps (|z - zmin| + tol z)  of  occlusion_tol z   (the subtraction, the product)
  T3  r - z (and so z - r) within  eps (|r| + |r - z| + tol z) + dz (1 + tol)  of  +-depth_tol z   (the division too),
      on pixels with A >= acc_min; A itself is an input and compares with acc_min exactly on both sides (bar 0)
  T5  one_per_pixel: the winner of a pixel and its runner-up when their z differ by no more than dz + dz' and the two
      points are not the same three floats (float32 may order them the other way)
  and, with one_per_pixel, every point in view that shares a pixel with a fragile point or lies in a pixel a P1 / P2
  point can reach (lidar_ref.bars' `keep`).
  C1  colour only: X or Y within dX / dY of an integer -- floor() may take the neighbouring cell, whose slope the
      sensitivity above does not know; the point's colour is not compared, everything else of it is.
The EXACT_CASES (identity pose, power-of-two focal lengths, dyadic coordinates, image values and fractions, tolerances
1/2 and 1/4, footprint 3/2 so that sigma = z / 4) have no rounding in any evaluation order: bit for bit, no bars, no
fragile set.
"""
import functools
import math

import numpy as np
import torch

import intrinsics as IX
import lidar_ref as L
import poses as PZ

F64 = torch.float64
EPS = L.EPS
ADMITTED, OUT, OCCLUDED, EXPLAINED, BEHIND, DUPLICATE = range(6)
OPTIONAL = ("depth", "acc", "lidar", "image", "covs", "exposure")


def _f32(v):
    return float(np.float32(v))


# ---- float64: the loop ---------------------------------------------------------------------------------------------
def _sample64(img, X, Y, H, W):
    """(value per channel, |dv/dX|, |dv/dY|, largest |tap|) of the bilinear sample with border replication."""
    x0, y0 = math.floor(X), math.floor(Y)
    tx, ty = X - x0, Y - y0
    xa, xb = min(max(x0, 0), W - 1), min(max(x0 + 1, 0), W - 1)
    ya, yb = min(max(y0, 0), H - 1), min(max(y0 + 1, 0), H - 1)
    out = []
    for c in range(3):
        v00, v01, v10, v11 = (float(img[c, ya, xa]), float(img[c, ya, xb]), float(img[c, yb, xa]),
                              float(img[c, yb, xb]))
        top = v00 + tx * (v01 - v00)
        bot = v10 + tx * (v11 - v10)
        out.append((top + ty * (bot - top), abs((1 - ty) * (v01 - v00) + ty * (v11 - v10)), abs(bot - top),
                    max(abs(v00), abs(v01), abs(v10), abs(v11))))
    return out


def admit64(x):
    """The contract of gsr_sweep_admit in float64.  x: the dict of inputs().  Returns codes [n] uint8, counts [6],
    and for the admitted points in input order: index, pixel, z, xyz, covs [m,9], rgb [m,3] (None without an image);
    and what bars() needs: proj (lidar_ref.project64's dict), ix, iy (-1 off view), zmin, r (NaN where not read),
    slope [m,3,3] = (|dv/dX|, |dv/dY|, V) per channel."""
    e = L.project64(x["points"], x["T_cw"], x["K"])
    n, H, W = e["x"].shape[0], x["H"], x["W"]
    lo, hi = x["min_depth"], x["max_depth"]
    lid, D, A, img = x.get("lidar"), x.get("depth"), x.get("acc"), x.get("image")
    tol_o, tol_d, amin, rad = _f32(x["occlusion_tol"]), _f32(x["depth_tol"]), _f32(x["acc_min"]), int(x["radius"])
    codes = np.zeros(n, np.uint8)
    ixs, iys = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    zmins, rs = np.full(n, np.nan), np.full(n, np.nan)
    winner = {}
    for i in range(n):
        codes[i] = OUT
        if not e["finite"][i]:
            continue
        z, X, Y = float(e["z"][i]), float(e["X"][i]), float(e["Y"][i])
        if z <= lo or z > hi or abs(X) > L.COORD_MAX or abs(Y) > L.COORD_MAX:
            continue
        ix, iy = math.floor(X + 0.5), math.floor(Y + 0.5)
        if ix < 0 or ix >= W or iy < 0 or iy >= H:
            continue
        ixs[i], iys[i] = ix, iy
        codes[i] = ADMITTED
        if lid is not None:
            zmin = None
            for v in range(max(iy - rad, 0), min(iy + rad, H - 1) + 1):
                for u in range(max(ix - rad, 0), min(ix + rad, W - 1) + 1):
                    q = float(lid[v, u])
                    if q > 0 and (zmin is None or q < zmin):
                        zmin = q
            if zmin is not None:
                zmins[i] = zmin
                if z - zmin > tol_o * z:
                    codes[i] = OCCLUDED
                    continue
        if D is not None:
            a = float(A[iy, ix])
            if a >= amin:
                with np.errstate(all="ignore"):
                    r = float(np.float64(D[iy, ix]) / np.float64(a))
                rs[i] = r
                if r - z > tol_d * z:
                    pass
                elif z - r > tol_d * z:
                    codes[i] = BEHIND
                    continue
                else:
                    codes[i] = EXPLAINED
                    continue
        if x["one_per_pixel"]:
            key = (z, i)
            p = iy * W + ix
            if p not in winner or key < winner[p]:
                winner[p] = key
    if x["one_per_pixel"]:
        for i in np.nonzero(codes == ADMITTED)[0]:
            if winner[int(iys[i]) * W + int(ixs[i])][1] != i:
                codes[i] = DUPLICATE
    index = np.nonzero(codes == ADMITTED)[0]
    m = index.shape[0]
    fsum = float(np.float32(np.asarray(x["K"]).reshape(3, 3)[0, 0])) + float(np.float32(np.asarray(x["K"]).reshape(3, 3)[1, 1]))
    z = e["z"][index]
    if x.get("covs") is not None:
        covs = np.asarray(x["covs"], np.float64).reshape(n, 9)[index]
    else:
        sigma = ((_f32(x["footprint"]) * z) * 2.0) / fsum
        covs = np.zeros((m, 9))
        covs[:, 0] = covs[:, 4] = covs[:, 8] = sigma * sigma
    rgb = slope = None
    if img is not None:
        rgb, slope = np.zeros((m, 3)), np.zeros((m, 3, 3))
        ex = x.get("exposure")
        for j, i in enumerate(index):
            for c, (v, sx, sy, V) in enumerate(_sample64(img, float(e["X"][i]), float(e["Y"][i]), H, W)):
                if ex is not None:
                    v = (v - float(ex[c, 1])) / float(ex[c, 0])
                rgb[j, c] = v * 255.0
                slope[j, c] = (sx, sy, V)
    return dict(codes=codes, counts=np.bincount(codes, minlength=6).astype(np.int64), index=index,
                pixel=iys[index] * W + ixs[index], z=z, xyz=np.asarray(x["points"])[index], covs=covs, rgb=rgb,
                proj=e, ix=ixs, iy=iys, zmin=zmins, r=rs, slope=slope)


# ---- the same in Torch ops -----------------------------------------------------------------------------------------
def admit_ops(x, dtype=F64, device="cpu"):
    """admit64's codes, counts, index, pixel, z, xyz, covs and rgb in Torch ops of one dtype on one device (tensors).
    The host composition the fused call replaces: one nonzero (a host wait) and the gathers behind it."""
    t = lambda a: L._tensor(a, dtype, device)  # noqa: E731
    pts = t(x["points"]).reshape(-1, 3)
    n, H, W = pts.shape[0], x["H"], x["W"]
    T, K = t(x["T_cw"]).reshape(-1, 4)[:3], t(x["K"]).reshape(3, 3)
    R, tr = T[:, :3], T[:, 3]
    p = [R[r, 0] * pts[:, 0] + R[r, 1] * pts[:, 1] + R[r, 2] * pts[:, 2] + tr[r] for r in range(3)]
    N = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
    X, Y, z = N[0] / N[2], N[1] / N[2], p[2]
    ok = torch.isfinite(pts).all(1) & torch.isfinite(z) & torch.isfinite(X) & torch.isfinite(Y)
    ok = ok & (z > x["min_depth"]) & (z <= x["max_depth"]) & (X.abs() <= L.COORD_MAX) & (Y.abs() <= L.COORD_MAX)
    X, Y = torch.where(ok, X, torch.zeros_like(X)), torch.where(ok, Y, torch.zeros_like(Y))
    ix, iy = torch.floor(X + 0.5).long(), torch.floor(Y + 0.5).long()
    ok = ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    pix = torch.where(ok, iy * W + ix, torch.zeros_like(ix))
    codes = torch.where(ok, 0, OUT).to(torch.uint8)
    live = ok
    tol_o, tol_d, amin = _f32(x["occlusion_tol"]), _f32(x["depth_tol"]), _f32(x["acc_min"])
    if x.get("lidar") is not None:
        lid = t(x["lidar"]).reshape(1, 1, H, W)
        far = torch.where(lid > 0, lid, torch.full_like(lid, float("inf")))
        k = 2 * int(x["radius"]) + 1       # (max_pool2d pads with -inf: the window clamped to the image)
        zmin = -torch.nn.functional.max_pool2d(-far, k, 1, k // 2).reshape(-1)[pix]
        occ = live & torch.isfinite(zmin) & (z - zmin > tol_o * z)
        codes = torch.where(occ, OCCLUDED, codes)
        live = live & ~occ
    if x.get("depth") is not None:
        D, A = t(x["depth"]).reshape(-1)[pix], t(x["acc"]).reshape(-1)[pix]
        sil = live & (A >= amin)
        r = D / torch.where(sil, A, torch.ones_like(A))
        front = r - z > tol_d * z
        behind = sil & ~front & (z - r > tol_d * z)
        expl = sil & ~front & ~behind
        codes = torch.where(behind, BEHIND, torch.where(expl, EXPLAINED, codes))
        live = live & ~behind & ~expl
    if x["one_per_pixel"]:
        slot = torch.where(live, pix, torch.full_like(pix, H * W))
        best = torch.full((H * W + 1,), float("inf"), dtype=dtype, device=device)
        best = best.scatter_reduce(0, slot, z, "amin", include_self=True)
        first = live & (z == best[slot])
        idx = torch.arange(n, device=device)
        low = torch.full((H * W + 1,), n, dtype=torch.long, device=device)
        low = low.scatter_reduce(0, torch.where(first, pix, torch.full_like(pix, H * W)), idx, "amin", include_self=True)
        dup = live & (low[slot] != idx)
        codes = torch.where(dup, DUPLICATE, codes)
        live = live & ~dup
    index = torch.nonzero(live).reshape(-1)
    zs = z[index]
    if x.get("covs") is not None:
        covs = t(x["covs"]).reshape(n, 9)[index]
    else:
        fsum = (K[0, 0] + K[1, 1]) if dtype == torch.float32 else _f32(x["K"][0][0]) + _f32(x["K"][1][1])
        sigma = ((_f32(x["footprint"]) * zs) * 2.0) / fsum
        covs = torch.zeros((index.shape[0], 9), dtype=dtype, device=device)
        covs[:, 0] = covs[:, 4] = covs[:, 8] = sigma * sigma
    rgb = None
    if x.get("image") is not None:
        img = t(x["image"]).reshape(3, H * W)
        Xs, Ys = X[index], Y[index]
        x0, y0 = torch.floor(Xs), torch.floor(Ys)
        tx, ty = (Xs - x0)[None], (Ys - y0)[None]
        x0, y0 = x0.long(), y0.long()
        xa, xb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
        ya, yb = y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
        v00, v01, v10, v11 = img[:, ya * W + xa], img[:, ya * W + xb], img[:, yb * W + xa], img[:, yb * W + xb]
        top = v00 + tx * (v01 - v00)
        bot = v10 + tx * (v11 - v10)
        v = top + ty * (bot - top)
        if x.get("exposure") is not None:
            ex = t(x["exposure"])
            v = (v - ex[:, 1:2]) / ex[:, 0:1]
        rgb = (v * 255.0).t().contiguous()
    return dict(codes=codes, counts=torch.bincount(codes.long(), minlength=6), index=index, pixel=pix[index], z=zs,
                xyz=pts[index], covs=covs, rgb=rgb)


# ---- bars and fragile points ---------------------------------------------------------------------------------------
def bars(x, t):
    """t: admit64(x).  fragile [n] bool; rgb_keep [m] bool; per admitted point the bars z [m], var [m], rgb [m,3]."""
    e, H, W = t["proj"], x["H"], x["W"]
    b = L.bars(e, H, W, x["min_depth"], x["max_depth"])
    n = e["x"].shape[0]
    z, dz, dX, dY = e["z"], b["dz"], b["dX"], b["dY"]
    inview = t["ix"] >= 0
    frag = (b["P1"] | b["P2"]).copy()
    tol_o, tol_d = _f32(x["occlusion_tol"]), _f32(x["depth_tol"])
    with np.errstate(all="ignore"):
        if x.get("lidar") is not None:
            gap = z - t["zmin"]
            bar = dz * (1 + tol_o) + EPS * (np.abs(gap) + tol_o * np.abs(z))
            frag |= inview & np.isfinite(t["zmin"]) & (np.abs(gap - tol_o * z) <= bar)
        if x.get("depth") is not None:
            r = t["r"]
            bar = EPS * (np.abs(r) + np.abs(r - z) + tol_d * np.abs(z)) + dz * (1 + tol_d)
            frag |= inview & np.isfinite(r) & ((np.abs(r - z - tol_d * z) <= bar) | (np.abs(z - r - tol_d * z) <= bar))
    pix = t["iy"] * W + t["ix"]
    if x["one_per_pixel"]:
        surv = np.nonzero((t["codes"] == ADMITTED) | (t["codes"] == DUPLICATE))[0]
        order = surv[np.lexsort((surv, z[surv], pix[surv]))]
        pts = np.asarray(x["points"])
        for a, c in zip(order[:-1], order[1:]):
            if pix[a] == pix[c] and t["codes"][a] == ADMITTED and z[c] - z[a] <= dz[a] + dz[c] \
                    and pts[a].tobytes() != pts[c].tobytes():
                frag[a] = frag[c] = True
        bad = ~b["keep"].reshape(-1)
        bad[pix[frag & inview]] = True
        frag |= inview & bad[np.where(inview, pix, 0)]
    idx = t["index"]
    fr = lambda v: np.abs(v - np.round(v))  # noqa: E731
    rgb_keep = ~((fr(e["X"][idx]) <= dX[idx]) | (fr(e["Y"][idx]) <= dY[idx]))
    zi = z[idx]
    var = t["covs"][:, 0] * (2 * dz[idx] / zi + 8 * EPS)
    rgb = None
    if t["rgb"] is not None:
        sx, sy, V = t["slope"][:, :, 0], t["slope"][:, :, 1], t["slope"][:, :, 2]
        dv = 14 * EPS * V + sx * dX[idx, None] + sy * dY[idx, None]
        if x.get("exposure") is not None:
            g = np.abs(np.asarray(x["exposure"], np.float64)[:, 0])[None]
            du = dv / g + 2 * EPS * np.abs(t["rgb"]) / 255.0
        else:
            du = dv
        rgb = 255.0 * du + EPS * np.abs(t["rgb"])
    assert frag.shape == (n,)
    return dict(fragile=frag, rgb_keep=rgb_keep, z=dz[idx], var=var, rgb=rgb)


# ---- the inputs of the tests ---------------------------------------------------------------------------------------
def _tiny_K():
    W, H, fx, fy = IX.INTRINSICS["tiny"][:4]
    assert (W, H) == (33, 17) and fx != fy
    return np.array([[fx, 0, (W - 1) / 2], [0, fy, (H - 1) / 2], [0, 0, 1]], np.float32)


# name -> (H, W, n, pose of poses.POSES / lidar_ref.POSES, intrinsics, seed, absent optional inputs, overrides).  Both
# image sizes; a posed camera (rpy, zup: every entry of R non-zero); fx != fy throughout (lidar_ref.intrinsics; the
# 33 x 17 camera is tests/intrinsics.py's "tiny"); each optional input present and absent; radius 0 .. 3; n <= 6000.
CASES = {
    "full_70x50": (50, 70, 6000, "identity", "lidar", 31, (), {}),
    "posed_70x50": (50, 70, 5000, "rpy", "lidar", 32, ("exposure",), dict(radius=2, footprint=1.5, covs=True)),
    "tiny_33x17": (17, 33, 1500, "zup", "tiny", 37, (), dict(radius=3, depth_tol=0.1)),
    "no_render_70x50": (50, 70, 4000, "yaw", "lidar", 34, ("depth", "acc"), dict(radius=0, near=0.5)),
    "no_lidar_33x17": (17, 33, 2000, "zup", "tiny", 35, ("lidar", "image", "exposure"), {}),
    "all_per_pixel_70x50": (50, 70, 3001, "rpy", "lidar", 36, ("exposure",), dict(one_per_pixel=False)),
}
# (the seeds are chosen so that the float64 reference alone keeps the fragile share under 1 %: with three points per
# pixel at 33 x 17 one point on a pixel's edge takes its pixel-mates with it; tests/test_seed_cases.py asserts it)
CASE_NAMES = tuple(CASES)
MIN_SHARE = 0.03


def possible_codes(x):
    """The codes a case's inputs enable (a code whose input is absent cannot occur: its rule is never evaluated)."""
    out = [ADMITTED, OUT]
    if x.get("lidar") is not None:
        out.append(OCCLUDED)
    if x.get("depth") is not None:
        out += [EXPLAINED, BEHIND]
    if x["one_per_pixel"]:
        out.append(DUPLICATE)
    return out


def _pose(name):
    R_cw, T = (L.POSES[name] if name in L.POSES else PZ.POSES[name])
    T_cw = np.concatenate([R_cw.T, (-R_cw.T @ T)[:, None]], 1).astype(np.float32)
    return R_cw, T, T_cw


def _far(u, v, H, W):
    """The far surface of the random scenes, as a depth over pixel coordinates."""
    return 4.0 + 0.6 * np.sin(u / W * 3.0) + 0.4 * np.cos(v / H * 2.0)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The float32 inputs of one of CASES or EXACT_CASES.
    Sweep: pixel coordinates from 8 % outside the image on every side; one point in sixteen behind the camera, one NaN
    and one Inf coordinate; on a smooth far surface (4 m +- 1 m, +- 2 cm of noise), but over the left 30 % of the
    image one in four (`near`: one in two) on a near surface (1.5 m) -- the far points behind it are seen through its gaps.
    lidar_depth: the sweep's own z-buffer (lidar_ref's float64 image, rounded once).
    Render: below 62 % of the height the map is missing (A in [0.05, 0.45]); above it A in [0.55, 1], D / A = the far
    surface at the pixel centre times 1 (half of the pixels), 1.3 (the render lies behind the measurement) or 0.7 (in
    front of it); a few pixels with A == acc_min exactly, one NaN in A and one in D.
    Image: a smooth pattern plus noise in 0 .. 1; exposure rows off the identity; covs: random positive diagonals."""
    if case in EXACT_CASES:
        return _exact_inputs(case)
    H, W, n, pname, kname, seed, absent, over = CASES[case]
    rng = np.random.default_rng(seed)
    K = L.intrinsics(H, W) if kname == "lidar" else _tiny_K()
    R_cw, T, T_cw = _pose(pname)
    K64 = K.astype(np.float64)
    u = rng.uniform(-0.08 * W - 0.5, 1.08 * W - 0.5, n)
    v = rng.uniform(-0.08 * H - 0.5, 1.08 * H - 0.5, n)
    near = (rng.uniform(0, 1, n) < over.get("near", 0.25)) & (u < 0.3 * W)
    z = np.where(near, 1.5 + 0.02 * rng.uniform(-1, 1, n), _far(u, v, H, W) + 0.02 * rng.uniform(-1, 1, n))
    z = np.where(rng.uniform(0, 1, n) < 1.0 / 16.0, -rng.uniform(0.3, 5.0, n), z)
    cam = np.stack([(u - K64[0, 2]) / K64[0, 0] * z, (v - K64[1, 2]) / K64[1, 1] * z, z], 1)
    pts = (cam @ R_cw.T + T).astype(np.float32).reshape(n, 3)
    pts[3, 0] = np.nan
    pts[5, 2] = np.inf
    x = dict(points=pts, T_cw=T_cw, K=K, H=H, W=W, n=n, min_depth=L.MIN_DEPTH, max_depth=L.MAX_DEPTH, exact=False,
             acc_min=0.5, depth_tol=_f32(0.05), occlusion_tol=_f32(0.1), radius=1, footprint=1.0, one_per_pixel=True)
    # (lidar_ref.image_ops in float64 equals image64 bit for bit -- tests/test_lidar_ref.py -- and needs no loop)
    lidar = L.image_ops(pts, T_cw, K, H, W, counts=False).numpy().astype(np.float32)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    hole = vv >= 0.62 * H
    A = np.where(hole, rng.uniform(0.05, 0.45, (H, W)), rng.uniform(0.55, 1.0, (H, W)))
    factor = rng.choice([1.0, 1.0, 1.3, 0.7], (H, W))
    D = A * _far(uu, vv, H, W) * factor
    A, D = A.astype(np.float32), D.astype(np.float32)
    A.reshape(-1)[::11][:7] = np.float32(0.5)
    A.reshape(-1)[17] = np.nan
    D.reshape(-1)[29] = np.nan
    image = 0.5 + 0.3 * np.sin(uu / 5.0)[None] * np.cos(vv / 4.0 + np.arange(3)[:, None, None]) \
        + 0.15 * rng.uniform(-1, 1, (3, H, W))
    exposure = np.array([[0.8, -0.05], [1.0, 0.0], [1.25, 0.1]], np.float32)
    covs = np.zeros((n, 9), np.float32)
    covs[:, [0, 4, 8]] = rng.uniform(1e-4, 1e-2, (n, 3)).astype(np.float32)
    covs[:, 1] = covs[:, 3] = 1e-5
    full = dict(depth=D, acc=A, lidar=lidar, image=image.astype(np.float32), exposure=exposure,
                covs=covs if over.get("covs") else None)
    for k in OPTIONAL:
        x[k] = None if k in absent else full[k]
    x.update({k: (_f32(val) if isinstance(val, float) else val) for k, val in over.items() if k not in ("covs", "near")})
    return x


# ---- the exact cases -------------------------------------------------------------------------------------------------
EXACT_CASES = {"exact_17x33": (17, 33, 600, 41), "exact_n0": (17, 33, 0, 42)}
EXACT_Z = (0.25, 1.0, 1.25, 1.5, 2.0, 2.5, 4.0, 16.0)   # min_depth itself (out) .. beyond max_depth; a few bits each
EXACT_NAMES = tuple(EXACT_CASES)


def _exact_inputs(case):
    """Dyadic everything (module docstring).  Random points over rows 0 .. H - 4 on a grid of quarter pixels, z one of
    EXACT_Z (1/4 == min_depth: out; 16: beyond max_depth == 8; between them steps that land on, inside and outside both
    tolerances); row H - 3 stays empty; row H - 1 carries, three
    pixels apart so that no occlusion window of radius 1 reaches a neighbour:
      z == min_depth (out), z == max_depth (in), z == 2 max_depth (out), X == -0.5 (pixel 0), X == W - 0.5 (out),
      A == acc_min with r == z (explained: >= ), r - z == depth_tol z (explained: the strict >), z - r == depth_tol z
      (explained), two identical points (the first admitted, the second a duplicate), z - zmin == occlusion_tol z (not
      occluded), z - zmin == 2 occlusion_tol z (occluded).
    Render over the random rows: A in {1/4, 1/2, 3/4, 1}, D / A in {1/2, 1, 3/2, 2, 3, 8}."""
    H, W, n, seed = EXACT_CASES[case]
    rng = np.random.default_rng(seed)
    K, lo, hi = L.EXACT_K, L.EXACT_MIN, L.EXACT_MAX
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    yb = float(H - 1)
    special = [(3.0, yb, lo), (6.0, yb, hi), (9.0, yb, 2 * hi), (-0.5, yb, 2.0), (W - 0.5, yb, 2.0), (12.0, yb, 2.0),
               (15.0, yb, 2.0), (18.25, yb, 2.0), (18.25, yb, 2.0), (21.0, yb, 2.0), (24.0, yb, 4.0), (25.0, yb, 3.0),
               (28.0, yb, 4.0), (29.0, yb, 2.0)]
    if n == 0:
        special = []
    k = len(special)
    X = rng.integers(-4, 4 * W + 2, n) / 4.0
    Y = rng.integers(-4, 4 * (H - 3) - 2, n) / 4.0                 # Y + 0.5 < H - 3: rows 0 .. H - 4
    z = rng.choice(EXACT_Z, n)
    for j, (sx, sy, sz) in enumerate(special):
        X[n - k + j], Y[n - k + j], z[n - k + j] = sx, sy, sz
    pts = np.stack([(X - cx) / fx * z, (Y - cy) / fy * z, z], 1)
    assert (pts.astype(np.float32).astype(np.float64) == pts).all()
    pts = pts.astype(np.float32).reshape(n, 3)
    lidar = L.image64(pts, L.EXACT_T, K, H, W, lo, hi)[0]
    assert (lidar.astype(np.float32).astype(np.float64) == lidar).all()
    A = rng.integers(1, 5, (H, W)) / 4.0
    r = rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 8.0], (H, W))
    A[H - 1, :] = 0.25                                              # the special row: no silhouette, except
    r[H - 1, :] = 1.0
    A[H - 1, 12], r[H - 1, 12] = 0.5, 2.0                           # A == acc_min, r == z
    A[H - 1, 15], r[H - 1, 15] = 1.0, 3.0                           # r - z == z / 2
    A[H - 1, 21], r[H - 1, 21] = 1.0, 1.0                           # z - r == z / 2
    image = rng.integers(0, 17, (3, H, W)) / 16.0
    exposure = np.array([[2.0, 0.25], [0.5, -0.125], [1.0, 0.0]], np.float32)
    return dict(points=pts, T_cw=L.EXACT_T, K=K, H=H, W=W, n=n, min_depth=lo, max_depth=hi, exact=True, acc_min=0.5,
                depth_tol=0.5, occlusion_tol=0.25, radius=1, footprint=1.5, one_per_pixel=True,
                depth=(A * r).astype(np.float32), acc=A.astype(np.float32), lidar=lidar.astype(np.float32),
                image=image.astype(np.float32), exposure=exposure, covs=None)


# what the special points of "exact_17x33" must come to (index from the end of the sweep -> code)
EXACT_SPECIAL_CODES = (OUT, ADMITTED, OUT, ADMITTED, OUT, EXPLAINED, EXPLAINED, ADMITTED, DUPLICATE, EXPLAINED,
                       ADMITTED, ADMITTED, OCCLUDED, ADMITTED)


@functools.lru_cache(maxsize=None)
def reference(case):
    """truth (admit64), the float32 yardstick (admit_ops), the final bars per admitted point of the truth, the fragile
    points.  Exact cases: the truth alone, every continuous output exactly a float32."""
    x = inputs(case)
    t = admit64(x)
    if x["exact"]:
        for k in ("z", "covs", "rgb"):
            assert (t[k].astype(np.float32).astype(np.float64) == t[k]).all(), k
        return dict(truth=t)
    y = admit_ops(x, torch.float32)
    b = bars(x, t)
    return dict(truth=t, f32=y, bars=b, fragile=b["fragile"], n_fragile=int(b["fragile"].sum()),
                final=final_bars(t, b, y))


def _by_index(t_index, g_index, g_values, width):
    """g_values (rows in the order of g_index) scattered to the rows of t_index; NaN where g lacks the point."""
    out = np.full((len(t_index), width), np.nan)
    pos = {int(i): j for j, i in enumerate(np.asarray(g_index).reshape(-1))}
    g = np.asarray(g_values, np.float64).reshape(len(pos), width) if len(pos) else np.zeros((0, width))
    for j, i in enumerate(t_index):
        if int(i) in pos:
            out[j] = g[pos[int(i)]]
    return out


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def final_bars(t, b, y):
    """max(2 e_ref, bar) per continuous output; e_ref = 0 where the yardstick does not admit the point."""
    out = {}
    for k, width, truth, bar in (("z", 1, t["z"], b["z"]), ("var", 1, t["covs"][:, 0], b["var"]),
                                 ("rgb", 3, t["rgb"], b["rgb"])):
        if truth is None:
            continue
        vals = _np(y["covs"])[:, 0] if k == "var" else _np(y[k])
        got = _by_index(t["index"], _np(y["index"]), vals, width)
        eref = np.nan_to_num(np.abs(got - np.asarray(truth, np.float64).reshape(-1, width)), nan=0.0)
        out[k] = np.maximum(2 * eref, np.asarray(bar, np.float64).reshape(-1, width))
    return out


def ratios(got, ref, x):
    """got: dict(codes [n], counts [6], index, pixel, z, covs [m,9], rgb or None) as arrays.  Returns the number of
    wrong codes off the fragile points, the worst count error against its slack (the fragile points), whether the
    admitted rows are the truth's off the fragile points (index, pixel, input order), and the worst |error| / bar of
    z, var and rgb over the compared points."""
    t, frag, fin = ref["truth"], ref["fragile"], ref["final"]
    codes = _np(got["codes"])
    out = dict(codes=int(((codes != t["codes"]) & ~frag).sum()))
    dc = np.abs(_np(got["counts"]).astype(np.int64) - t["counts"])
    out["counts"] = float(dc.max() / ref["n_fragile"]) if ref["n_fragile"] else (0.0 if dc.max() == 0 else 1e9)
    gi = _np(got["index"]).astype(np.int64)
    keep_t, keep_g = ~frag[t["index"]], ~frag[gi]
    out["rows"] = bool(np.array_equal(gi[keep_g], t["index"][keep_t]) and (np.diff(gi) > 0).all()
                       and np.array_equal(_np(got["pixel"]).astype(np.int64)[keep_g], t["pixel"][keep_t]))
    for k, width, truth in (("z", 1, t["z"]), ("var", 1, t["covs"][:, 0]), ("rgb", 3, t["rgb"])):
        if truth is None or (k == "var" and x.get("covs") is not None):
            continue
        vals = _np(got["covs"])[:, 0] if k == "var" else _np(got[k])
        g = _by_index(t["index"], gi, vals, width)
        d = np.abs(g - np.asarray(truth, np.float64).reshape(-1, width))
        keep = keep_t & (ref["bars"]["rgb_keep"] if k == "rgb" else True)
        d = np.where(np.isfinite(d), d, 1e30)     # (a compared point the other side lacks, or a NaN: fails)
        out[k] = L._ratio(d, fin[k], keep[:, None])
    return out


# ---- the end-to-end scene --------------------------------------------------------------------------------------------
HOLE = (26, 48, 14, 34)        # u0, u1, v0, v1: pixels [u0, u1) x [v0, v1) of the 70 x 50 image have no Gaussian
SURFACE_Z = 4.5
E2E = dict(depth_tol=0.05, occlusion_tol=0.1, footprint=1.0, acc_min=0.5)


@functools.lru_cache(maxsize=1)
def hole_scene():
    """A surface the size of tests/iteration.py's scene -- 600 Gaussians (a 30 x 20 lattice) seen at 70 x 50 by its
    camera 0 -- on the plane z = 4.5 m of its sweep, flat along z, opacity 1/2 and identity rotation as
    add_new_pointcloud leaves them; the rows that project into HOLE are removed.  And a sweep of two points per pixel
    sampled from the FULL surface.  -> dict(xyz, scales, rgbs (0..255), sweep, K, T_cw, H, W, in_hole(pixel))."""
    import iteration as IT
    W, H = IT.W, IT.H
    K = IT.raster_K()
    rng = np.random.default_rng(77)
    # (the lattice reaches two pixels past the image on every side, so that the border pixels are covered too)
    gu, gv = np.meshgrid((np.arange(30) + 0.5) * (W + 4) / 30 - 2.5, (np.arange(20) + 0.5) * (H + 4) / 20 - 2.5)
    gu, gv = gu.reshape(-1), gv.reshape(-1)
    u0, u1, v0, v1 = HOLE
    keep = ~((gu >= u0) & (gu < u1 - 1) & (gv >= v0) & (gv < v1 - 1))
    back = lambda u, v, z: np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)  # noqa: E731
    xyz = back(gu, gv, np.full(gu.shape, SURFACE_Z))[keep].astype(np.float32)
    s = 1.6 * SURFACE_Z / K[0, 0]                                   # 1.6 pixels
    scales = np.tile(np.array([s, s, 0.01], np.float32), (xyz.shape[0], 1))
    rgbs = rng.uniform(40, 220, (xyz.shape[0], 3)).astype(np.float32)
    n = 2 * W * H
    su, sv = rng.uniform(-0.5, W - 0.5, n), rng.uniform(-0.5, H - 0.5, n)
    sweep = back(su, sv, SURFACE_Z + 0.02 * rng.uniform(-1, 1, n)).astype(np.float32)
    return dict(xyz=xyz, scales=scales, rgbs=rgbs, sweep=sweep, K=K, T_cw=IT.world_to_camera(0), H=H, W=W)


def in_hole(pixel, W=70):
    u0, u1, v0, v1 = HOLE
    pixel = np.asarray(pixel)
    return (pixel % W >= u0) & (pixel % W < u1) & (pixel // W >= v0) & (pixel // W < v1)


def oracle_scene(xyz, scales, rgbs):
    """The oracle's scene dict of rows as add_new_pointcloud initialises them, under iteration's camera 0."""
    import iteration as IT
    P = xyz.shape[0]
    sc = dict(IT.cameras()[0])
    sc.update(means3D=np.asarray(xyz, np.float32), scales=np.asarray(scales, np.float32),
              rotations=np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1)), opacities=np.full((P, 1), 0.5, np.float32),
              shs=((np.asarray(rgbs, np.float32) / 255.0 - 0.5) / 0.28209479177387814)[:, None, :].astype(np.float32),
              sh_degree=0, bg=np.zeros(3, np.float32), scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None,
              W=IT.W, H=IT.H)
    return sc
