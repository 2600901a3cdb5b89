"""Reference of the per-Gaussian blend contribution (gsr_contribution): CPU, numpy, test infrastructure only.

per_gaussian(fr) walks every tile's list of an oracle frame (oracle.oracle.forward) as the blend does.  The CUTS -- which
(pixel, splat) pairs are blended -- are decided in float32 on the frame's own means2D / conic_opacity, the oracle's
expression, with `index < n_contrib[pixel]` as the termination (tests/ref64.blend does the same with its `cut=`
argument); the WEIGHTS alpha * T are carried in float64.  A pixel the oracle flags `fragile` may legitimately decide a
cut differently in another float32 implementation, so it is left out of the sums and widens the count of every row of
its tile instead: lo <= n_touched <= hi.

yardstick32(fr) takes the same walk entirely in float32 in the forward's order: how far a float32 implementation is from
the float64 weights before a hardware exp2 or a pre-scaled conic adds anything.
"""
import math

import numpy as np

from gs_livm_amd import synthetic as S

TILE = 16
F32 = np.float32
# worst |yardstick32 - float64| / float64 of weight_sum and weight_max over SCENES (measured: 7.62e-7 and 5.36e-7 on the
# largest; tests/test_contrib_ref.py holds the reference to it).  The GPU comparison allows B = 8 x this: the margin
# covers the hardware exp2 and the pre-scaled conic, which the yardstick's libm exp form does not have.
YARDSTICK = 7.7e-7
B = 8.0 * YARDSTICK


def _tile_pixels(fr, t):
    gx = (fr.W + TILE - 1) // TILE
    ty, tx = divmod(t, gx)
    ys, xs = np.meshgrid(np.arange(ty * TILE, min(ty * TILE + TILE, fr.H)),
                         np.arange(tx * TILE, min(tx * TILE + TILE, fr.W)), indexing="ij")
    return ys.ravel(), xs.ravel()


def _tile_walk(fr, t):
    """(ids [L], ys, xs [n], take [n, L] bool, alpha32 [n, L], power-inputs) of tile t: the float32 cuts."""
    lo, hi = int(fr.ranges[t, 0]), int(fr.ranges[t, 1])
    ids = fr.point_list[lo:hi].astype(np.int64)
    ys, xs = _tile_pixels(fr, t)
    m2, co = fr.means2D[ids], fr.conic_opacity[ids]
    dx = m2[None, :, 0] - xs[:, None].astype(F32)
    dy = m2[None, :, 1] - ys[:, None].astype(F32)
    # gsr_oracle.c, blend_tile: -0.5f * (A dx dx + C dy dy) - B dx dy, every operation rounded to float32
    power = F32(-0.5) * (co[None, :, 0] * dx * dx + co[None, :, 2] * dy * dy) - co[None, :, 1] * dx * dy
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        alpha = np.minimum(F32(0.99), co[None, :, 3] * np.exp(power, dtype=F32))
    index = np.arange(len(ids))[None, :]
    take = (index < fr.n_contrib[ys, xs][:, None].astype(np.int64)) & ~(power > 0) & ~(alpha < F32(1.0 / 255.0))
    return ids, ys, xs, take, alpha, (dx, dy, co)


def per_gaussian(fr):
    """dict of [P] arrays: lo, hi (int64), wsum64, wmax64 (float64, over non-fragile pixels), tiles (int64)."""
    P = fr.P
    lo_n, amb = np.zeros(P, np.int64), np.zeros(P, np.int64)
    wsum, wmax, tiles = np.zeros(P), np.zeros(P), np.zeros(P, np.int64)
    for t in range(fr.ranges.shape[0]):
        ids, ys, xs, take, _, (dx, dy, co) = _tile_walk(fr, t)
        if len(ids) == 0:
            continue
        dx, dy, co = dx.astype(np.float64), dy.astype(np.float64), co.astype(np.float64)
        power = -0.5 * (co[None, :, 0] * dx * dx + co[None, :, 2] * dy * dy) - co[None, :, 1] * dx * dy
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.where(take, np.minimum(0.99, co[None, :, 3] * np.exp(power)), 0.0)
        T = np.cumprod(np.concatenate([np.ones_like(a[:, :1]), 1.0 - a[:, :-1]], 1), 1)
        w = a * T
        ok = fr.fragile[ys, xs] == 0
        np.add.at(tiles, ids, 1)
        np.add.at(amb, ids, int((~ok).sum()))
        np.add.at(lo_n, ids, take[ok].sum(0))
        np.add.at(wsum, ids, w[ok].sum(0))
        np.maximum.at(wmax, ids, w[ok].max(0, initial=0.0))
    return dict(lo=lo_n, hi=lo_n + amb, wsum64=wsum, wmax64=wmax, tiles=tiles)


def yardstick32(fr):
    """dict of [P] float32 arrays wsum32, wmax32 over non-fragile pixels: the walk in float32 throughout, T carried as
    the forward carries it (T <- T * (1 - alpha)), a tile's pixels added in float32, the tiles added in float64 (the
    fixed-point accumulation adds them exactly)."""
    P = fr.P
    wsum, wmax = np.zeros(P), np.zeros(P, F32)
    for t in range(fr.ranges.shape[0]):
        ids, ys, xs, take, alpha, _ = _tile_walk(fr, t)
        if len(ids) == 0:
            continue
        a = np.where(take, alpha, F32(0))
        T = np.cumprod(np.concatenate([np.ones_like(a[:, :1]), F32(1) - a[:, :-1]], 1), 1, dtype=F32)
        w = (a * T).astype(F32)
        ok = fr.fragile[ys, xs] == 0
        np.add.at(wsum, ids, w[ok].sum(0, dtype=F32).astype(np.float64))
        np.maximum.at(wmax, ids, w[ok].max(0, initial=F32(0)))
    return dict(wsum32=wsum.astype(F32), wmax32=wmax)


def worst_ratio(got, ref):
    """max |got - ref| / ref over the rows with ref > 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = ref > 0
    return float((np.abs(got[m] - ref[m]) / ref[m]).max(initial=0.0))


# ---- scenes -------------------------------------------------------------------------------------------------------
SCENES = [(300, 70, 50, 11, 3), (7, 33, 17, 3, 1), (2500, 257, 131, 4, 2)]


def scene(P, W, H, seed, D):
    return S.make_scene(P, W, H, seed, sh_degree=D)


def splat_scene(W, H, centers_px, depths, sigma_px, opacity, fovx_deg=60.0):
    """Isotropic Gaussians whose projections are centred on the given pixel coordinates with (about) sigma_px pixels of
    standard deviation before the rasterizer's 0.3 px^2 low-pass, at the given view-space depths (row order = depth order
    when the depths increase)."""
    cam = S.make_camera(W, H, fovx_deg=fovx_deg)
    n = len(depths)
    z = np.asarray(depths, np.float64)
    c = np.asarray(centers_px, np.float64).reshape(n, 2)
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    ndc = (2.0 * c + 1.0) / np.array([W, H]) - 1.0  # ndc2Pix inverted
    means = np.stack([ndc[:, 0] * cam["tanfovx"] * z, ndc[:, 1] * cam["tanfovy"] * z, z], 1)
    s = sigma_px * z / math.sqrt(fx * fy)
    assert s.max(initial=0.0) <= 0.3, "beyond the rasterizer's scale cull"
    sc = dict(cam)
    sc.update(means3D=means.astype(F32), scales=np.repeat(s[:, None], 3, 1).astype(F32),
              rotations=np.tile(np.array([1, 0, 0, 0], F32), (n, 1)),
              opacities=np.full((n, 1), opacity, F32), shs=np.full((n, 1, 3), 0.5, F32), sh_degree=0,
              bg=np.zeros(3, F32), scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None)
    return sc


def stack_scene(N, opacity, W=16, H=16, sigma_px=100.0):
    """One tile, N identical Gaussians one behind the other: a narrow field of view makes their footprint (sigma = 100 px)
    flat over the tile, so every pixel sees alpha = min(0.99, opacity * G) with G >= 0.994.  A small sigma_px instead makes
    the stack opaque in the middle of the tile and open at its border: the pixels stop at different list positions."""
    z = 1.0 + 0.001 * np.arange(N)
    return splat_scene(W, H, np.tile([[7.5, 7.5]], (N, 1)), z, sigma_px, opacity, fovx_deg=2.0)


def ellipse_pixels(fr, row, clip=True):
    """(count, weight sum) of the closed form opacity * exp(-1/2 (A dx^2 + C dy^2) - B dx dy) >= 1/255 over the pixel
    lattice of the image (float64 on the frame's own 2-D values), and the smallest relative distance of a pixel's alpha
    from the cut."""
    A, B, C, o = (float(v) for v in fr.conic_opacity[row])
    cx, cy = (float(v) for v in fr.means2D[row])
    ys, xs = np.mgrid[0:fr.H, 0:fr.W] if clip else np.mgrid[-64:fr.H + 64, -64:fr.W + 64]
    dx, dy = cx - xs, cy - ys
    alpha = np.minimum(0.99, o * np.exp(-0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy))
    inside = alpha >= 1.0 / 255.0
    margin = float(np.abs(alpha * 255.0 - 1.0).min())
    return int(inside.sum()), float(alpha[inside].sum()), margin
