"""References for the depth gradient of the blend backward (gsr_backward_depth): test infrastructure, CPU only.

The rendered depth is depth(p) = sum_i z_i alpha_i(p) T_i(p) with z_i the view-space depth of Gaussian i.  A loss on it
reaches the Gaussians two ways: through alpha (z is one more "colour" of the splat) and directly through z_i, hence
through the mean.  Two independent restatements:

* render64: float64, composed from ref64's own pieces (per_gaussian, project, blend, gaussian_vjp) with the depth a
  differentiable LEAF of each tile's blend.  The loss is sum c g_c + sum acc g_a + sum depth g_d; every gradient is
  torch.autograd's, no backward formula is written.  Returns ref64.render's dict plus dL_ddepths [P] (dL/dz_i) and, with
  slack=True, ref64's slack extended to the depth leaf: the exact gradient at the frame's f32 depths, means2D, conic and
  colour minus the exact gradient at the exact values.
* yardstick32: float32 numpy, pixel by pixel and list entry by list entry in the FORM of the reference's backward
  (backward.cu:533-571: one "what lies behind" recurrence per colour channel and one for the silhouette, with the
  background term added separately), plus a fifth recurrence for the depth and the direct term.  It shares no
  structure with the kernels' one-recurrence form; it says what an honest float32 evaluation achieves against render64
  and so anchors the bar the GPU tests use (tests/test_depth_ref.py).  It yields the five groups the blend produces:
  dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors, dL_ddepths.

SCENES / MIXES are the cases tests/test_gpu_depth_grad.py runs; reference(name, mix) evaluates one of them once per
process.
"""
import functools

import numpy as np
import torch

import poses as PO
import ref64 as R
from gs_livm_amd import synthetic as S
from helpers import masked_upstream, ref64_path_scene
from oracle import oracle as O

NAMES2 = ("ndc", "conic", "opacity", "color", "depth")
GRAD_NAMES = R.GRAD_NAMES + ("dL_ddepths",)
BLEND_GROUPS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_ddepths")

# name -> (P, W, H, seed, SH degree) | path of helpers.REF64_PATHS | (pose of poses.POSES)
PLAIN = {"P7_33x17": (7, 33, 17, 3, 1), "P1_64x64": (1, 64, 64, 2, 0), "P300_70x50": (300, 70, 50, 11, 3),
         "P2500_257x131": (2500, 257, 131, 5, 2)}
PATHS = ("colors_precomp", "cov3D_precomp", "opaque", "scale_modifier")
POSED = ("rpy", "zup")
# (the 2 500-Gaussian scene with seed 5, not REF64_SCENES' 4: on seed 4 the float32 yardstick itself sits at 0.51 of the
# bar for dL_dopacity under a depth-only loss -- z g_d minus what lies behind cancels where the depths of a tile are close --
# and the scene changes, not the bar; DESIGN.md section 2 has the ratios)
SCENES = tuple(PLAIN) + PATHS + tuple("pose_" + p for p in POSED)
MIXES = ("all", "depth_only", "no_depth")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, seed) of one of SCENES."""
    if name in PLAIN:
        P, W, H, seed, D = PLAIN[name]
        return S.make_scene(P, W, H, seed, sh_degree=D), seed
    if name in PATHS:
        return ref64_path_scene(name)
    pose = name[len("pose_"):]
    return PO.posed(S.make_scene(1500, 200, 120, 13, sh_degree=3), *PO.POSES[pose]), 13  # tests/test_poses.py's MAIN


def upstream(sc, fr, seed, mix):
    """(g_c (3, H, W), g_a (1, H, W), g_d (1, H, W)) float32: masked_upstream's colour and silhouette gradients and
    seeded uniform noise in [-1, 1] / (largest view-space depth of the frame) for the depth, all zero on fragile
    pixels; mix 'depth_only' zeroes g_c and g_a, 'no_depth' zeroes g_d."""
    W, H = sc["W"], sc["H"]
    dcol, dacc = masked_upstream(W, H, seed, fr.fragile)
    vis = fr.radii > 0
    zmax = float(fr.depths[vis].max()) if vis.any() else 1.0
    gd = np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, (1, H, W)) / zmax
    gd = (gd * (fr.fragile == 0)[None]).astype(np.float32)
    if mix == "depth_only":
        dcol, dacc = np.zeros_like(dcol), np.zeros_like(dacc)
    elif mix == "no_depth":
        gd = np.zeros_like(gd)
    else:
        assert mix == "all", mix
    return dcol, dacc, gd


def _blend_frame(sc, fr, vis, vals, g_c, g_a, g_d, departures):
    """ref64._blend_frame with the depth as the fifth leaf of every tile's graph and depth . g_d in the loss: the f64
    gradients with respect to the 2-D leaves and the depth (rows vis)."""
    P, W, H = fr.P, fr.W, fr.H
    vt = torch.as_tensor(vis)
    full = {}
    for k, shp in (("ndc", (P, 2)), ("conic", (P, 3)), ("opacity", (P,)), ("color", (P, 3)), ("depth", (P,))):
        full[k] = torch.zeros(shp, dtype=R.F64)
        full[k][vt] = vals[k].detach()
    bg = R._t(sc["bg"])
    m2, co32 = R._t(fr.means2D), R._t(fr.conic_opacity[:, :3])
    dcol, dacc, ddep = R._t(g_c).reshape(3, H * W), R._t(g_a).reshape(H * W), R._t(g_d).reshape(H * W)
    acc_g = {k: torch.zeros_like(full[k]) for k in NAMES2}
    for tidx in range(fr.ranges.shape[0]):
        lo, hi = int(fr.ranges[tidx, 0]), int(fr.ranges[tidx, 1])
        if hi == lo:
            continue
        ys, xs = R._tile_pixels(fr, tidx)
        pid = torch.as_tensor(ys * W + xs)
        ids = torch.as_tensor(fr.point_list[lo:hi].astype(np.int64))
        leaves = [full[k][ids].clone().requires_grad_(True) for k in NAMES2]
        c, d, a, _, _ = R.blend(W, H, R._t(xs), R._t(ys), *leaves, bg, departures, cut=(m2[ids], co32[ids]))
        loss = (c * dcol[:, pid].T).sum() + (a * dacc[pid]).sum() + (d * ddep[pid]).sum()
        for k, gr in zip(NAMES2, torch.autograd.grad(loss, leaves, allow_unused=True)):
            if gr is not None:
                acc_g[k].index_add_(0, ids, gr)
    return {k: acc_g[k][vt] for k in NAMES2}


def _to_3d(sc, fr, vis, g2, departures):
    """The per-Gaussian stage: ref64.gaussian_vjp for the four 2-D groups, plus autograd's VJP of the view-space depth
    (ref64.project's third output) for dL/dz; scattered into the reference's arrays, dL_ddepths added."""
    g3 = R.gaussian_vjp(sc, vis, fr.clamped, g2, departures)
    leaves, out = R.per_gaussian(sc, vis, fr.clamped, departures)
    (gm,) = torch.autograd.grad(out["depth"], [leaves["means3D"]], g2["depth"])
    g3["means3D"] = g3["means3D"] + gm
    o = R.expand_grads(sc, fr, vis, g2, g3)
    o["dL_ddepths"] = np.zeros(fr.P)
    o["dL_ddepths"][vis] = g2["depth"].numpy()
    return o


def render64(sc, fr, g_c, g_a, g_d, departures=True, slack=False):
    """Float64 gradients of sum c g_c + sum acc g_a + sum depth g_d (module docstring)."""
    vis = np.flatnonzero(fr.radii > 0)
    with torch.no_grad():
        _, vals = R.per_gaussian(sc, vis, fr.clamped, departures)
    g2 = _blend_frame(sc, fr, vis, vals, g_c, g_a, g_d, departures)
    out = _to_3d(sc, fr, vis, g2, departures)
    if slack:
        v32 = dict(vals)
        wh = torch.tensor([fr.W, fr.H], dtype=R.F64)
        v32["ndc"] = (2.0 * R._t(fr.means2D[vis]) + 1.0) / wh - 1.0
        v32["conic"] = R._t(fr.conic_opacity[vis, :3])
        v32["depth"] = R._t(fr.depths[vis])
        if sc.get("colors_precomp") is None:
            v32["color"] = R._t(fr.rgb[vis])
        g2b = _blend_frame(sc, fr, vis, v32, g_c, g_a, g_d, departures)
        d = _to_3d(sc, fr, vis, {k: g2[k] - g2b[k] for k in g2}, departures)
        out["slack"] = {k: np.abs(d[k]) for k in GRAD_NAMES}
    return out


def yardstick32(sc, fr, g_c, g_a, g_d):
    """Float32 blend backward in the reference's form (module docstring).  Every pixel of a tile walks the tile's list
    back to front; the pixels of a tile are the elements of the arrays below, each with its own state, and every
    operation is a float32 operation.  Per-Gaussian sums are float32, tile by tile."""
    f = np.float32
    P, W, H = fr.P, fr.W, fr.H
    bg = np.asarray(sc["bg"], f)
    xy, co, col, z = fr.means2D.astype(f), fr.conic_opacity.astype(f), fr.rgb.astype(f), fr.depths.astype(f)
    if sc.get("colors_precomp") is not None:
        col = np.asarray(sc["colors_precomp"], f)
    g_c, g_a, g_d = (np.asarray(a, f).reshape(-1, H * W) for a in (g_c, g_a, g_d))
    ddx, ddy = f(0.5 * W), f(0.5 * H)
    out = {"dL_dmeans2D": np.zeros((P, 3), f), "dL_dconic": np.zeros((P, 2, 2), f), "dL_dopacity": np.zeros((P, 1), f),
           "dL_dcolors": np.zeros((P, 3), f), "dL_ddepths": np.zeros(P, f)}
    half, one = f(0.5), f(1.0)
    for tidx in range(fr.ranges.shape[0]):
        lo, hi = int(fr.ranges[tidx, 0]), int(fr.ranges[tidx, 1])
        if hi == lo:
            continue
        ys, xs = R._tile_pixels(fr, tidx)
        pid = ys * W + xs
        px, py = xs.astype(f), ys.astype(f)
        T_final = fr.final_T.reshape(-1)[pid].astype(f)
        last = fr.n_contrib.reshape(-1)[pid].astype(np.int64)
        dp, da, dd = g_c[:, pid], g_a[0, pid], g_d[0, pid]
        T = T_final.copy()
        acc_c = np.zeros((3, pid.size), f)      # accum_rec
        acc_a = np.zeros(pid.size, f)           # accum_acc_rec
        acc_z = np.zeros(pid.size, f)           # accum_depth_rec
        last_alpha = np.zeros(pid.size, f)
        last_c = np.zeros((3, pid.size), f)
        last_a = np.zeros(pid.size, f)
        last_z = np.zeros(pid.size, f)
        bg_dot = (bg[0] * dp[0] + bg[1] * dp[1]) + bg[2] * dp[2]
        for pos in range(hi - lo - 1, -1, -1):
            gid = int(fr.point_list[lo + pos])
            dx, dy = xy[gid, 0] - px, xy[gid, 1] - py
            A, B, C, o = co[gid]
            power = -half * (A * dx * dx + C * dy * dy) - B * dx * dy
            G = np.exp(power, dtype=f)
            alpha = np.minimum(f(0.99), o * G)
            take = (pos < last) & ~(power > 0) & ~(alpha < f(1.0 / 255.0))
            if not take.any():
                continue
            a_t = np.where(take, alpha, f(0))
            Tn = np.where(take, T / (one - a_t), T)
            dch = a_t * Tn
            dL_dalpha = np.zeros(pid.size, f)
            for ch in range(3):
                c = col[gid, ch]
                new = last_alpha * last_c[ch] + (one - last_alpha) * acc_c[ch]
                acc_c[ch] = np.where(take, new, acc_c[ch])
                last_c[ch] = np.where(take, c, last_c[ch])
                dL_dalpha = dL_dalpha + (c - acc_c[ch]) * dp[ch]
                out["dL_dcolors"][gid, ch] += (dch * dp[ch]).sum(dtype=f)
            new = last_alpha * last_a + (one - last_alpha) * acc_a
            acc_a = np.where(take, new, acc_a)
            last_a = np.where(take, one, last_a)
            dL_dalpha = dL_dalpha + (one - acc_a) * da
            new = last_alpha * last_z + (one - last_alpha) * acc_z
            acc_z = np.where(take, new, acc_z)
            last_z = np.where(take, z[gid], last_z)
            dL_dalpha = dL_dalpha + (z[gid] - acc_z) * dd
            out["dL_ddepths"][gid] += (dch * dd).sum(dtype=f)
            dL_dalpha = dL_dalpha * Tn
            last_alpha = np.where(take, alpha, last_alpha)
            dL_dalpha = dL_dalpha + (-T_final / (one - a_t)) * bg_dot
            dL_dalpha = np.where(take, dL_dalpha, f(0))
            T = Tn
            dL_dG = o * dL_dalpha
            gdx, gdy = G * dx, G * dy
            dG_dx = -gdx * A - gdy * B
            dG_dy = -gdy * C - gdx * B
            out["dL_dmeans2D"][gid, 0] += (dL_dG * dG_dx * ddx).sum(dtype=f)
            out["dL_dmeans2D"][gid, 1] += (dL_dG * dG_dy * ddy).sum(dtype=f)
            out["dL_dconic"][gid, 0, 0] += (-half * gdx * dx * dL_dG).sum(dtype=f)
            out["dL_dconic"][gid, 0, 1] += (-half * gdx * dy * dL_dG).sum(dtype=f)
            out["dL_dconic"][gid, 1, 1] += (-half * gdy * dy * dL_dG).sum(dtype=f)
            out["dL_dopacity"][gid, 0] += (G * dL_dalpha).sum(dtype=f)
    return out


@functools.lru_cache(maxsize=None)
def frame(name):
    """The f32 oracle frame of a scene: the discrete structure, the fragile map and the f32 2-D values."""
    sc, _ = scene(name)
    O.set_threads(min(O.max_threads(), 16))
    return O.forward(sc)


@functools.lru_cache(maxsize=None)
def reference(name, mix):
    """(scene, frame, (g_c, g_a, g_d), render64(..., slack=True)) of one case, evaluated once per process."""
    sc, seed = scene(name)
    fr = frame(name)
    up = upstream(sc, fr, seed, mix)
    return sc, fr, up, render64(sc, fr, *up, slack=True)


def ratios(got, r, names):
    """{group: worst |d| / bar}, the bar being helpers.grad_close's with slack= (a row of dL_ddepths is its element)."""
    out = {}
    for k in names:
        ref = r[k].reshape(np.shape(got[k]))
        if ref.size == 0:
            continue
        P = ref.shape[0]
        shape = (P,) + (1,) * (ref.ndim - 1)
        tol = 1e-5 * float(np.abs(ref).max()) + 1e-4 * np.abs(ref.reshape(P, -1)).max(1).reshape(shape)
        tol = tol + r["slack"][k].reshape(P, -1).max(1).reshape(shape)
        out[k] = float((np.abs(got[k] - ref) / np.maximum(tol, 1e-300)).max())
    return out
