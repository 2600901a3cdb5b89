"""Scenes that sit ON the rasterizer's discrete decisions, and scenes that hold non-finite values (test infrastructure).

make_gaussians draws depths, scales and opacities from continuous ranges: no input of the other modules ever lands on a
cull boundary, and none holds a NaN or an Inf.  Two families here, shared by tests/test_nonfinite.py (the CPU oracle)
and tests/test_gpu_nonfinite.py (the HIP path):

BOUNDARIES  one small scene per decision, two Gaussians ONE FLOAT APART (np.nextafter in float32), with the outcome
            written out from the reference's source line -- not taken from the oracle.  Camera: yaw 0 at the origin, so
            the view-space depth IS the mean's z; odd image sizes (33 x 17), so an on-axis mean projects onto the centre
            of pixel (16, 8) exactly: dx = dy = 0, power == 0, exp == 1, alpha == opacity there.
POISONS     make_scene(300, 65, 49, SEED) -- two k_preprocess blocks, the second one partial -- at degree 0 and through
            sh_layouts.with_layout at degree 3, with NaN / +Inf / -Inf written into one field of one row, of all of
            POISON_ROWS, or (everything()) into every field at once on different rows.
"""
import functools

import numpy as np

import intrinsics as IX
import sh_layouts as L
from gs_livm_amd import synthetic as S

F = np.float32
W0, H0, CX, CY = 33, 17, 16, 8          # boundary scenes: image size and the pixel an on-axis mean lands on
BG = np.array([0.125, 0.75, 0.25], F)   # uniform background, far from COLOUR
DC = np.array([1.5, -1.5, 1.0], F)      # SH dc of the boundary rows
C0 = F(0.28209479177387814)
COLOUR = (C0 * DC + F(0.5)).astype(F)   # forward.cu:29-76 at degree 0: C0 * dc + 0.5 in f32
INV255 = F(1.0) / F(255.0)              # the kernels' 1.0f / 255.0f


def up(x):
    return np.nextafter(F(x), F(np.inf), dtype=F)


def down(x):
    return np.nextafter(F(x), F(-np.inf), dtype=F)


def _rows(cam, means, scales, opac, dc=None, **extra):
    n = len(means)
    shs = np.zeros((n, 1, 3), F)
    shs[:, 0] = DC if dc is None else dc
    sc = dict(cam, means3D=np.asarray(means, F).reshape(n, 3), scales=np.asarray(scales, F).reshape(n, 3),
              rotations=np.tile(np.array([1, 0, 0, 0], F), (n, 1)), opacities=np.asarray(opac, F).reshape(n, 1), shs=shs,
              sh_degree=0, bg=BG.copy(), scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None)
    sc.update(extra)
    return sc


def _cam():
    return S.make_camera(W0, H0)


# ---- boundary scenes -------------------------------------------------------------------------------------------------
# Every builder returns (scene, expect): expect["visible"][i] says whether row i has radii > 0 (and, where it does and
# "tiles" is not given otherwise, tiles_touched > 0 in both binning modes); further keys are read by the tests that
# know them.  Row 0 is the value ON the decision, row 1 its float neighbour on the other side.

def near_cull():
    """forward.cu:221-225 via auxiliary.h:120-144: `if (p_view.z <= 0.2f) return false` -- 0.2f itself is culled."""
    z0, z1 = F(0.2), up(0.2)
    sc = _rows(_cam(), [[0, 0, z0], [0, 0, z1]], [[0.004] * 3] * 2, [0.5, 0.5])
    return sc, dict(visible=[False, True])


def scale_modifier_pair(mod=0.7):
    """Raw scales (a, up(a)) whose float32 products with `mod` fall on 0.3f or below / above it: chosen by evaluating
    the kernels' own f32 multiply on the CPU."""
    mod, lim = F(mod), F(0.3)
    a = F(lim / mod)
    while F(mod * a) > lim:
        a = down(a)
    while F(mod * up(a)) <= lim:
        a = up(a)
    assert F(mod * a) <= lim < F(mod * up(a))
    return a, up(a)


def scale_cull(component, mod=1.0):
    """forward.cu:19-25, 227-229: culled iff some mod * scale component > 0.3f -- 0.3f itself is kept."""
    keep, cull = (F(0.3), up(0.3)) if mod == 1.0 else scale_modifier_pair(mod)
    s = np.full((2, 3), 0.05, F)
    s[0, component], s[1, component] = keep, cull
    sc = _rows(_cam(), [[0, 0, 6.0], [0, 0, 6.0]], s, [0.5, 0.5], scale_modifier=float(mod))
    return sc, dict(visible=[True, False])


def alpha_cut(which):
    """forward.cu:374-376: `if (alpha < 1.0f / 255.0f) continue` -- alpha == 1/255 contributes.  ONE Gaussian whose
    centre pixel has alpha == opacity; which = 0: opacity 1/255 (in), 1: the float below it (out)."""
    op = INV255 if which == 0 else down(INV255)
    sc = _rows(_cam(), [[0, 0, 4.0]], [[0.05] * 3], [op])
    centre = (BG * (F(1.0) - op) + op * COLOUR).astype(F) if which == 0 else BG
    return sc, dict(visible=[True], contributes=(which == 0), centre=centre, opacity=op)


def alpha_clamp():
    """forward.cu:373: alpha = min(0.99f, opacity * exp(power)): final_T of the centre pixel is 1 - 0.99f."""
    sc = _rows(_cam(), [[0, 0, 4.0]], [[0.05] * 3], [1.0])
    return sc, dict(visible=[True], final_T=F(1.0) - F(0.99))


def indefinite_cov():
    """A finite cov3D_precomp whose 2-D covariance is indefinite after the low-pass: cxx + 0.3 < 0 < cyy + 0.3.  det < 0
    (kept: forward.cu:243 tests det == 0), the conic has a negative xx term, so power > 0 along x (skipped,
    forward.cu:367-368) and <= 0 along the centre column (blended).  Row 1 is an ordinary splat behind it."""
    cov = np.array([[-0.02, 0, 0, 0.01, 0, 0.01], [0.01, 0, 0, 0.01, 0, 0.01]], F)
    sc = _rows(_cam(), [[0, 0, 2.0], [0.1, 0.05, 3.0]], [[0.05] * 3] * 2, [0.7, 0.6], cov3D_precomp=cov)
    sc["scales"] = sc["rotations"] = None
    return sc, dict(visible=[True, True])


def det_zero():
    """forward.cu:243 `if (det == 0.0f) return`: fx = fy = z = 16 makes the Jacobian the identity (W / (2 tanfovx) with
    tanfovx = 33/32 is 16 exactly), so Sigma_xx = -0.3f gives cxx + 0.3f == 0 and, with Sigma_xy = 0, det == 0.0f.  Row 1
    is one float towards zero: det is a tiny positive number and the row is kept."""
    cam = IX.camera(W0, H0, 16.0, 16.0)
    cov = np.array([[F(-0.3), 0, 0, 0.01, 0, 0.01], [up(-0.3), 0, 0, 0.01, 0, 0.01]], F)
    sc = _rows(cam, [[0, 0, 16.0], [0, 0, 16.0]], [[0.05] * 3] * 2, [0.5, 0.5], cov3D_precomp=cov)
    sc["scales"] = sc["rotations"] = None
    return sc, dict(visible=[False, True])


BOUNDARIES = {"near": near_cull, "alpha_in": lambda: alpha_cut(0), "alpha_out": lambda: alpha_cut(1),
              "alpha_clamp": alpha_clamp, "indefinite": indefinite_cov, "det_zero": det_zero}
for _k in range(3):
    BOUNDARIES["scale%d" % _k] = functools.partial(scale_cull, _k)
    BOUNDARIES["scale%d_mod" % _k] = functools.partial(scale_cull, _k, 0.7)


def centre_upstream():
    """dL_dcolor that is non-zero at the centre pixel only (and no silhouette gradient)."""
    dcol = np.zeros((3, H0, W0), F)
    dcol[:, CY, CX] = (0.5, -0.25, 1.0)
    return dcol, np.zeros((1, H0, W0), F)


# ---- poisoned scenes -------------------------------------------------------------------------------------------------
PW, PH, PP = 65, 49, 300
# A seed at which the ORACLE's fragile fraction stays under the suites' 0.5 % on every scene below
# (tests/test_nonfinite.py asserts it).
SEED = 41
POISON_ROWS = (0, 255, 256, PP - 1)     # block 0's first and last row, block 1's first, and the row the duplicate lanes
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}       # of the partial block re-evaluate
# field -> (scene key, index inside the row); "rest" exists at degree 3 only
FIELDS = {"mean_x": ("means3D", (0,)), "mean_z": ("means3D", (2,)), "scale": ("scales", (1,)),
          "rotation": ("rotations", (2,)), "opacity": ("opacities", (0,)), "sh_dc": ("shs", (0, 1)),
          "sh_rest": ("shs", (9, 2)), "cov3D": ("cov3D_precomp", (3,)), "colour": ("colors_precomp", (1,))}


# Where the poisoned rows sit.  A row whose alpha is NaN blends at min(0.99, NaN) = 0.99 over every tile it has, and two
# such rows over one pixel give test_T = (1 - 0.99f)^2 = 0.99999e-4 -- ON the reference's T < 1e-4 stop, which the
# oracle rightly flags fragile.  So every poisoned row gets a full tile of its own: centred on it, a needle of sigma
# 2.1 px by the low-pass's 0.55 px, 3-sigma radius 7 (one tile under the reference's rectangle).  Laid DIAGONALLY the
# needle leaves the square's other two corners more than 14.4 minor sigmas away: there exp(power) has underflowed to 0,
# and those are the only pixels an opacity of -Inf paints (-Inf * 0 = NaN -> 0.99).  The ring just inside them, where
# exp(power) is subnormal, is decided by the exp implementation alone and is fragile (oracle/gsr_oracle.c, blend_tile):
# ten pixels per diagonal needle, which is why POISON_ROWS holds ONE (row 256, the row the single-row -Inf case hits).
FULL_TILES = [(tx, ty) for ty in range(PH // 16) for tx in range(PW // 16)]      # the 4 x 3 tiles of 16 x 16 pixels
ROW_TILES = {0: (0, 0), 255: (2, 0), 256: (1, 2), PP - 1: (3, 1)}
DIAGONAL_ROW = 256


def _place(sc, row, tile, diagonal, z=4.0):
    px, py = 16 * tile[0] + 7.5, 16 * tile[1] + 7.5
    sc["means3D"][row] = (((2 * px + 1) / PW - 1) * sc["tanfovx"] * z, ((2 * py + 1) / PH - 1) * sc["tanfovy"] * z, z)
    # (along x the minor sigma is 0.69 px: exp(power) stays normal over the whole square, no pixel is decided by exp)
    sc["scales"][row] = (0.15, 0.004, 0.004) if diagonal else (0.15, 0.03, 0.03)
    # (45 degrees about the optical axis, or none: the needle lies along x)
    sc["rotations"][row] = (0.9238795, 0.0, 0.0, 0.3826834) if diagonal else (1.0, 0.0, 0.0, 0.0)
    sc["opacities"][row] = 0.8


@functools.lru_cache(maxsize=None)
def _base(D):
    sc = S.make_scene(PP, PW, PH, SEED) if D == 0 else L.with_layout(PP, PW, PH, SEED, 3, 16)
    for r, tile in ROW_TILES.items():
        _place(sc, r, tile, r == DIAGONAL_ROW)
    return sc


def base(D):
    """A private copy of the unpoisoned scene at SH degree D (0 or 3)."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _base(D).items()}


def _route(sc, field):
    """Switch the scene to the input route `field` needs (precomputed covariances / colours of the clean scene)."""
    if field == "cov3D":
        from oracle import oracle as O
        fr = O.forward(sc, keep_handle=False)
        cov = fr.cov3D.copy()
        cov[fr.radii <= 0] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], F)
        sc["cov3D_precomp"], sc["scales"], sc["rotations"] = cov, None, None
    elif field == "colour":
        rng = np.random.default_rng(SEED + 1)
        sc["colors_precomp"], sc["shs"] = rng.uniform(0, 1, (PP, 3)).astype(F), None
    return sc


def poisoned(D, field, value, rows):
    """(scene, clean scene of the same route, rows) with VALUES[value] in `field` of `rows`."""
    clean = _route(base(D), field)
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    key, idx = FIELDS[field]
    for r in rows:
        sc[key][(r,) + idx] = VALUES[value]
    return sc, clean, tuple(rows)


def cases(D):
    """[(field, value, rows)]: every field x value on ONE row (the rows of POISON_ROWS in turn, so that each is hit by
    every value) and on ALL of POISON_ROWS."""
    out, i = [], 0
    for field in FIELDS:
        if field == "sh_rest" and D == 0:
            continue
        for value in VALUES:
            out.append((field, value, (POISON_ROWS[i % 4],)))
            out.append((field, value, POISON_ROWS))
            i += 1
    return out


def everything(D):
    """All poisons at once: every field of the scales / rotations / SH route x every value, each on a row of its own --
    POISON_ROWS first, then the rows after them -- and each row on a tile of FULL_TILES in turn (the first six, the
    means, are culled: no tile holds two rows that paint at 0.99).  Returns (scene, clean scene, rows)."""
    clean = base(D)
    rows = list(POISON_ROWS) + [r for r in range(1, PP) if r not in POISON_ROWS]
    plan = [(f, v) for f in FIELDS if f not in ("cov3D", "colour") and not (f == "sh_rest" and D == 0) for v in VALUES]
    for k in range(len(plan)):
        _place(clean, rows[k], FULL_TILES[k % len(FULL_TILES)], plan[k][0] == "opacity")
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    for k, (field, value) in enumerate(plan):
        key, idx = FIELDS[field]
        sc[key][(rows[k],) + idx] = VALUES[value]
    return sc, clean, tuple(rows[:len(plan)])


def reached_pixels(fr, rows):
    """(H, W) mask of the pixels inside the tiles that the frame's instances of `rows` lie in.  (A poisoned frame is
    compared with the clean one outside the union of both frames' masks: the clean frame still paints the row.)"""
    gx = (fr.W + 15) // 16
    hit = np.isin(fr.point_list, np.asarray(rows, np.uint32))
    tiles = np.unique((fr.keys[hit] >> np.uint64(32)).astype(np.int64))
    m = np.zeros((((fr.H + 15) // 16) * 16, gx * 16), bool)
    for t in tiles:
        m[(t // gx) * 16:(t // gx) * 16 + 16, (t % gx) * 16:(t % gx) * 16 + 16] = True
    return m[:fr.H, :fr.W]


def same(a, b):
    """bit-for-bit equality of float arrays where NaN equals NaN (x86 and the GPU differ in the NaN's sign bit)."""
    return np.array_equal(a, b, equal_nan=True)
