"""Float64 restatement of the rasterizer's forward, differentiated by torch.autograd only (CPU, test infrastructure).

Independent of oracle/gsr_oracle.c and of the HIP kernels: no backward formula is written here.  Every gradient
is autograd's derivative of the forward restated below, except where the reference's backward is knowingly not
the exact derivative of its forward.  Each such departure is modelled by a straight-through term and cites its
line (paths relative to the reference's src/cuda_rasterizer/ and include/gs/cuda_rasterizer/):

  D1  alpha = min(0.99, o*G): the clamp is not differentiated, d alpha = d(o*G)      (backward.cu:542, 584, 600)
  D2  dL_d{a,b,c} use denom2inv = 1/(denom^2 + 1e-7) instead of 1/denom^2            (backward.cu:203-212)
  D3  under the Jacobian clamp at 1.3*tanfov the clamped t.x = lim*t.z is a constant
      in the t.z terms of J; only x_grad_mul zeroes dL/dt.x                          (backward.cu:173-174, 262-266)
  D4  dL_dscales is the gradient with respect to s = scale_modifier * scale, not
      scale (the factor scale_modifier is never applied)                             (backward.cu:318, 340-342)

Conventions of the reference's gradient arrays (not departures):
  dL_dmeans2D[:, :2]  gradient with respect to the NDC position (pixel = ndc2Pix(ndc), d pix / d ndc = 0.5 W / 0.5 H,
                      backward.cu:505-506); column 2 is zero
  dL_dconic[:, 0, 1]  half of dL/dB for power = -0.5 (A dx^2 + C dy^2) - B dx dy; [:, 1, 0] is unused (zero)
  dL_dcov3D           gradient with respect to the 6-vector (xx, xy, xz, yy, yz, zz): off-diagonals counted twice

Discrete structure comes from an f32 oracle frame (oracle.oracle.Frame), which the HIP path reproduces bit for bit:
the visible set (radii > 0), each tile's ordered Gaussian list (point_list / ranges) and the SH clamp flags.  The
per-pixel cuts (power > 0, alpha < 1/255, T * (1 - alpha) < 1e-4) are decided here in f64 under no_grad; pixels where
f32 and f64 may legitimately decide a cut differently are the oracle's `fragile` ones.

Memory: the chain rule is split at the 2-D boundary (exact).  Per tile, the tile's NDC xy, conic, opacity and colour
are leaves of a small graph (the blend of that tile); their gradients accumulate per Gaussian; then one VJP of the
per-Gaussian stage (gaussian_vjp) maps them to the 3-D parameters.
"""
import numpy as np
import torch

F64 = torch.float64
TILE = 16

# SH basis constants (auxiliary.h:22-33)
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)

GRAD_NAMES = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
              "dL_dscales", "dL_drotations")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def straight_through(value, grad_like):
    """Value of `value`, gradient of `grad_like`."""
    return grad_like - (grad_like - value).detach()


def sh_to_rgb(deg, sh, means, campos, clamped=None):
    """forward.cu:29-76.  sh (n, M, 3), means (n, 3).  Colours are max(res + 0.5, 0); where `clamped` (the f32
    frame's flags, forward.cu:72-74) is given it decides the clamp, else the f64 sign does."""
    d = means - campos
    d = d / torch.sqrt((d * d).sum(1, keepdim=True))
    x, y, z = (d[:, k:k + 1] for k in range(3))
    res = SH_C0 * sh[:, 0]
    if deg > 0:
        res = res - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            res = (res + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * sh[:, 6]
                   + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
            if deg > 2:
                res = (res + SH_C3[0] * y * (3 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
                       + SH_C3[2] * y * (4 * zz - xx - yy) * sh[:, 11]
                       + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
                       + SH_C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
                       + SH_C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    res = res + 0.5
    cl = (res < 0) if clamped is None else clamped
    return torch.where(cl, torch.zeros_like(res), res)


def cov3d(scales, rotations, mod, departures=True):
    """forward.cu:138-176: M = S R with S = diag(mod * scale) and R from the quaternion (r, x, y, z) AS GIVEN (not
    normalised, forward.cu:146); Sigma = M^T M; returns the upper triangle (xx, xy, xz, yy, yz, zz)."""
    s = mod * scales
    if departures:  # D4 (backward.cu:340-342): dL_dscale is dL/ds, the factor mod is not applied
        s = straight_through(s, scales)
    r, x, y, z = rotations.unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], -1),
                     torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], -1),
                     torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    M = s[:, :, None] * R
    Sg = M.transpose(1, 2) @ M
    return torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1)


def camera(sc):
    W, H = int(sc["W"]), int(sc["H"])
    tx, ty = float(sc["tanfovx"]), float(sc["tanfovy"])
    return dict(W=W, H=H, tanx=tx, tany=ty, fx=W / (2.0 * tx), fy=H / (2.0 * ty), V=_t(sc["viewmatrix"]),
                Pm=_t(sc["projmatrix"]), campos=_t(sc["campos"]))


def project(cam, means, c6, departures=True):
    """Per-Gaussian 2-D stage from means (n, 3) and the 3-D covariance 6-vector c6 (n, 6).
    Returns ndc (n, 2), conic (n, 3) = (A, B, C), depth (n,).

    Matrices are column-major 4x4 in memory (auxiliary.h:48-64), so with the numpy (4, 4) view m,
    view-space t = p @ m[:3, :3] + m[3, :3] and the clip-space point is p @ P[:3] + P[3]."""
    V, Pm = cam["V"], cam["Pm"]
    t = means @ V[:3, :3] + V[3, :3]
    ph = means @ Pm[:3] + Pm[3]
    pw = 1.0 / (ph[:, 3:4] + 1e-7)                      # forward.cu:232-233
    ndc = ph[:, :2] * pw
    tx, ty, tz = t.unbind(1)
    limx, limy = 1.3 * cam["tanx"], 1.3 * cam["tany"]   # forward.cu:86-91 (EWA, computeCov2D)
    txtz, tytz = tx / tz, ty / tz
    cx = txtz.clamp(-limx, limx) * tz
    cy = tytz.clamp(-limy, limy) * tz
    if departures:  # D3 (backward.cu:173-174, 262-266): a clamped t.x is a constant wherever J uses it
        with torch.no_grad():
            ox, oy = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
        cx = torch.where(ox, cx.detach(), cx)
        cy = torch.where(oy, cy.detach(), cy)
    fx, fy = cam["fx"], cam["fy"]
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * cx / (tz * tz)], -1),
                     torch.stack([zero, fy / tz, -fy * cy / (tz * tz)], -1)], -2)          # (n, 2, 3)
    Rv = V[:3, :3].T                                    # t = Rv p + V[3, :3]
    c0, c1, c2, c3, c4, c5 = c6.unbind(1)
    Sig = torch.stack([torch.stack([c0, c1, c2], -1), torch.stack([c1, c3, c4], -1), torch.stack([c2, c4, c5], -1)],
                      -2)
    JW = J @ Rv
    cov = JW @ Sig @ JW.transpose(1, 2)
    a = cov[:, 0, 0] + 0.3                              # low-pass, forward.cu:130-131
    b = cov[:, 0, 1]
    c = cov[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c, -b, a], 1) / det[:, None]   # forward.cu:238-244
    if departures:  # D2 (backward.cu:203): the backward divides by denom^2 + 1e-7
        d2 = (det * det).detach()
        conic = straight_through(conic, conic * (d2 / (d2 + 1e-7))[:, None])
    return ndc, conic, tz


def per_gaussian(sc, idx, clamped=None, departures=True, leaves=None):
    """The whole per-Gaussian stage for the rows idx of the scene, from f64 leaves (created here unless given).
    Returns (leaves, out) with out = dict(ndc, conic, opacity, color, depth, cov6)."""
    cam = camera(sc)
    idx = torch.as_tensor(np.asarray(idx, np.int64))
    if leaves is None:
        leaves = {}
        for k in ("means3D", "scales", "rotations", "opacities", "shs", "colors_precomp", "cov3D_precomp"):
            v = sc.get(k)
            if v is not None and np.asarray(v).size:
                leaves[k] = _t(np.asarray(v)[idx.numpy()]).requires_grad_(True)
    mod = float(sc.get("scale_modifier", 1.0))
    if "cov3D_precomp" in leaves:
        c6 = leaves["cov3D_precomp"]
    else:
        c6 = cov3d(leaves["scales"], leaves["rotations"], mod, departures)
    ndc, conic, depth = project(cam, leaves["means3D"], c6, departures)
    if "colors_precomp" in leaves:
        color = leaves["colors_precomp"]
    else:
        cl = None if clamped is None else torch.as_tensor(np.asarray(clamped)[idx.numpy()].astype(bool))
        color = sh_to_rgb(int(sc["sh_degree"]), leaves["shs"], leaves["means3D"], cam["campos"], cl)
    return leaves, dict(ndc=ndc, conic=conic, opacity=leaves["opacities"][:, 0], color=color, depth=depth, cov6=c6)


def _power(mx, my, conic, pix_x, pix_y):
    dx = mx[None, :] - pix_x[:, None]
    dy = my[None, :] - pix_y[:, None]
    A, B, C = conic[:, 0], conic[:, 1], conic[:, 2]
    return -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy


def blend(W, H, pix_x, pix_y, ndc, conic, opacity, color, depth, bg, departures=True, cut=None):
    """forward.cu:291-407 for the pixels (pix_x, pix_y) (n_pix,) over one ordered list of Gaussians (L,): returns
    colour (n_pix, 3), depth (n_pix,), acc (n_pix,), final T (n_pix,), n_contrib (n_pix,).

    cut: None, or (means2D (L, 2), conic (L, 3)) of the f32 frame: the cuts are then decided in f64 arithmetic on
    those values -- the ones the HIP path blends with, bit for bit -- so that f32 and f64 can disagree on a cut only
    where the f32 blend's own rounding decides it, which is what the oracle's `fragile` map flags.  (Decided on the
    exact f64 positions instead, a cut can flip wherever the f32 rounding of means2D, ~1e-5 px at a few hundred px,
    moves alpha across 1/255: observed at non-fragile pixels.)"""
    mx = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5            # ndc2Pix, auxiliary.h:35-37
    my = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    power = _power(mx, my, conic, pix_x, pix_y)
    raw = opacity * torch.exp(power)
    alpha = torch.clamp(raw, max=0.99)
    if departures:  # D1 (backward.cu:542, 584, 600): dL_dG = o * dL_dalpha, dL_do = G * dL_dalpha, clamped or not
        alpha = straight_through(alpha, raw)
    with torch.no_grad():  # the cuts (forward.cu:357-383), decided in f64
        if cut is None:
            cp, ca = power, alpha
        else:
            cp = _power(cut[0][:, 0], cut[0][:, 1], cut[1], pix_x, pix_y)
            ca = torch.clamp(opacity * torch.exp(cp), max=0.99)
        a = torch.where((cp <= 0) & (ca >= 1.0 / 255.0), ca, torch.zeros_like(ca))
        keep = (a > 0) & ~(torch.cumprod(1.0 - a, 1) < 1e-4)
        n_contrib = torch.where(keep, torch.arange(1, a.shape[1] + 1).expand_as(a), 0).max(1).values \
            if a.shape[1] else torch.zeros(a.shape[0], dtype=torch.int64)
    a = alpha * keep
    one_m = 1.0 - a
    T = torch.cumprod(torch.cat([torch.ones_like(one_m[:, :1]), one_m[:, :-1]], 1), 1)
    w = a * T
    T_final = T[:, -1] * one_m[:, -1] if a.shape[1] else torch.ones(a.shape[0], dtype=F64)
    out_color = w @ color + T_final[:, None] * bg[None, :]
    return out_color, w @ depth, w.sum(1), T_final, n_contrib


def _tile_pixels(fr, tidx):
    gx = (fr.W + TILE - 1) // TILE
    ty, tx = divmod(tidx, gx)
    ys, xs = np.meshgrid(np.arange(ty * TILE, min(ty * TILE + TILE, fr.H)),
                         np.arange(tx * TILE, min(tx * TILE + TILE, fr.W)), indexing="ij")
    return ys.ravel(), xs.ravel()


def _blend_frame(sc, fr, vis, vals, dL_dcolor, dL_dacc, departures):
    """The blend of every tile of fr with the per-Gaussian values vals (rows vis); with upstream gradients also
    their f64 gradients with respect to the 2-D leaves (rows vis)."""
    P, W, H = fr.P, fr.W, fr.H
    vt = torch.as_tensor(vis)
    full = {}
    for k, shp in (("ndc", (P, 2)), ("conic", (P, 3)), ("opacity", (P,)), ("color", (P, 3)), ("depth", (P,))):
        full[k] = torch.zeros(shp, dtype=F64)
        full[k][vt] = vals[k].detach()
    bg = _t(sc["bg"])
    m2, co32 = _t(fr.means2D), _t(fr.conic_opacity[:, :3])
    want_grad = dL_dcolor is not None
    names = ("ndc", "conic", "opacity", "color")
    if want_grad:
        dcol = _t(dL_dcolor).reshape(3, H * W)
        dacc = _t(dL_dacc).reshape(H * W)
        acc_g = {k: torch.zeros_like(full[k]) for k in names}
    img = torch.zeros((3, H * W), dtype=F64)
    dep, acc = torch.zeros(H * W, dtype=F64), torch.zeros(H * W, dtype=F64)
    fT, nc = torch.ones(H * W, dtype=F64), torch.zeros(H * W, dtype=torch.int64)
    for tidx in range(fr.ranges.shape[0]):
        ys, xs = _tile_pixels(fr, tidx)
        pid = torch.as_tensor(ys * W + xs)
        lo, hi = int(fr.ranges[tidx, 0]), int(fr.ranges[tidx, 1])
        ids = torch.as_tensor(fr.point_list[lo:hi].astype(np.int64))
        leaves = [full[k][ids].clone().requires_grad_(want_grad) for k in names]
        with torch.set_grad_enabled(want_grad):
            c, d, a, t, n = blend(W, H, _t(xs), _t(ys), *leaves, full["depth"][ids], bg, departures,
                                  cut=(m2[ids], co32[ids]))
        img[:, pid], dep[pid], acc[pid], fT[pid], nc[pid] = c.detach().T, d.detach(), a.detach(), t.detach(), n
        if want_grad and len(ids):
            loss = (c * dcol[:, pid].T).sum() + (a * dacc[pid]).sum()
            grads = torch.autograd.grad(loss, leaves, allow_unused=True)
            for k, gr in zip(names, grads):
                if gr is not None:
                    acc_g[k].index_add_(0, ids, gr)
    out = dict(out_color=img.reshape(3, H, W).numpy(), out_depth=dep.reshape(1, H, W).numpy(),
               out_acc=acc.reshape(1, H, W).numpy(), final_T=fT.reshape(H, W).numpy(),
               n_contrib=nc.reshape(H, W).numpy())
    return out, ({k: acc_g[k][vt] for k in names} if want_grad else None)


def render(sc, fr, dL_dcolor=None, dL_dacc=None, departures=True, slack=False):
    """Forward (and, given upstream gradients, the backward) of one frame against the discrete structure of the f32
    oracle frame fr.  Returns a dict: out_color (3, H, W), out_depth (1, H, W), out_acc (1, H, W), final_T (H, W),
    n_contrib (H, W), and with upstream gradients the nine gradient groups in the reference's shapes (oracle.backward).

    slack=True adds 'slack': for each gradient group, per element, how far the exact gradient moves when the blend is
    evaluated at the f32 frame's 2-D values (means2D, conic, colour: what an f32 backward is handed) instead of the
    exact ones, propagated to the 3-D groups by the same VJP.  Both evaluations are f64; an f32 implementation may
    differ from the exact gradient by that much before its own arithmetic adds anything (see row_slack)."""
    vis = np.flatnonzero(fr.radii > 0)
    with torch.no_grad():
        _, vals = per_gaussian(sc, vis, fr.clamped, departures)
    out, g2 = _blend_frame(sc, fr, vis, vals, dL_dcolor, dL_dacc, departures)
    if g2 is None:
        return out
    out.update(expand_grads(sc, fr, vis, g2, gaussian_vjp(sc, vis, fr.clamped, g2, departures)))
    if slack:
        v32 = dict(vals)
        wh = torch.tensor([fr.W, fr.H], dtype=F64)
        v32["ndc"] = (2.0 * _t(fr.means2D[vis]) + 1.0) / wh - 1.0     # ndc2Pix inverted, exact in f64
        v32["conic"] = _t(fr.conic_opacity[vis, :3])
        if sc.get("colors_precomp") is None:
            v32["color"] = _t(fr.rgb[vis])
        _, g2b = _blend_frame(sc, fr, vis, v32, dL_dcolor, dL_dacc, departures)
        d2 = {k: g2[k] - g2b[k] for k in g2}
        d = expand_grads(sc, fr, vis, d2, gaussian_vjp(sc, vis, fr.clamped, d2, departures))
        out["slack"] = {k: np.abs(d[k]) for k in GRAD_NAMES}
    return out


def gaussian_vjp(sc, idx, clamped, g2, departures=True):
    """One VJP of the per-Gaussian stage for the rows idx, given upstream gradients g2 = dict(ndc (n, 2),
    conic (n, 3) = dL/d(A, B, C), opacity (n,), color (n, 3)).  Returns f64 dL/d of every 3-D input present and
    'cov6' (dL/d of the covariance 6-vector)."""
    leaves, out = per_gaussian(sc, idx, clamped, departures)
    c6 = out["cov6"]
    # split at the 6-vector so that dL_dcov3D comes out as well (exact: one more level of the chain rule)
    c6_leaf = c6.detach().clone().requires_grad_(True)
    cam = camera(sc)
    ndc, conic, _ = project(cam, leaves["means3D"], c6_leaf, departures)
    outs, ups = [ndc, conic], [g2["ndc"], g2["conic"]]
    if "colors_precomp" not in leaves:
        outs.append(out["color"])
        ups.append(g2["color"])
    wrt = [leaves["means3D"], c6_leaf] + [leaves[k] for k in ("shs",) if k in leaves]
    gr = torch.autograd.grad(outs, wrt, ups, allow_unused=True)
    res = {"means3D": gr[0], "cov6": gr[1]}
    if "shs" in leaves:
        res["shs"] = gr[2] if gr[2] is not None else torch.zeros_like(leaves["shs"])
    res["opacities"] = g2["opacity"][:, None]
    if "colors_precomp" in leaves:
        res["colors_precomp"] = g2["color"]
    if "scales" in leaves and "cov3D_precomp" not in leaves:
        gs, gq = torch.autograd.grad(c6, [leaves["scales"], leaves["rotations"]], res["cov6"])
        res["scales"], res["rotations"] = gs, gq
    for k in res:
        if res[k] is None:
            res[k] = torch.zeros_like(leaves[k])
    return res


def expand_grads(sc, fr, vis, g2, g3):
    """Scatter the f64 gradients of the visible rows into the reference's nine arrays (oracle.backward's shapes)."""
    P = fr.P
    M = 0 if sc.get("shs") is None or np.asarray(sc["shs"]).size == 0 else int(np.asarray(sc["shs"]).shape[1])
    o = {"dL_dmeans2D": np.zeros((P, 3)), "dL_dconic": np.zeros((P, 2, 2)), "dL_dopacity": np.zeros((P, 1)),
         "dL_dcolors": np.zeros((P, 3)), "dL_dmeans3D": np.zeros((P, 3)), "dL_dcov3D": np.zeros((P, 6)),
         "dL_dsh": np.zeros((P, M, 3)), "dL_dscales": np.zeros((P, 3)), "dL_drotations": np.zeros((P, 4))}
    cg = g2["conic"].numpy()
    o["dL_dmeans2D"][vis, :2] = g2["ndc"].numpy()
    o["dL_dconic"][vis, 0, 0] = cg[:, 0]
    o["dL_dconic"][vis, 0, 1] = 0.5 * cg[:, 1]
    o["dL_dconic"][vis, 1, 1] = cg[:, 2]
    o["dL_dopacity"][vis] = g2["opacity"].numpy()[:, None]
    o["dL_dcolors"][vis] = g2["color"].numpy()
    o["dL_dmeans3D"][vis] = g3["means3D"].numpy()
    o["dL_dcov3D"][vis] = g3["cov6"].numpy()
    if "shs" in g3:
        o["dL_dsh"][vis] = g3["shs"].numpy()
    if "scales" in g3:
        o["dL_dscales"][vis] = g3["scales"].numpy()
        o["dL_drotations"][vis] = g3["rotations"].numpy()
    return o


def upstream_from_reference_arrays(g, idx):
    """The reference's 2-D gradient arrays (HIP or oracle output, rows idx) as gaussian_vjp upstream, in f64."""
    cg = np.asarray(g["dL_dconic"], np.float64).reshape(-1, 2, 2)[idx]
    return {"ndc": _t(np.asarray(g["dL_dmeans2D"])[idx, :2]),
            "conic": _t(np.stack([cg[:, 0, 0], 2.0 * cg[:, 0, 1], cg[:, 1, 1]], 1)),
            "opacity": _t(np.asarray(g["dL_dopacity"]).reshape(-1)[idx]),
            "color": _t(np.asarray(g["dL_dcolors"])[idx])}


def beyond_jacobian_clamp(sc, idx):
    """True where a Gaussian's view-space mean lies beyond the 1.3 * tanfov Jacobian clamp (either axis)."""
    cam = camera(sc)
    t = _t(np.asarray(sc["means3D"])[idx]) @ cam["V"][:3, :3] + cam["V"][3, :3]
    return ((t[:, 0] / t[:, 2]).abs() > 1.3 * cam["tanx"]) | ((t[:, 1] / t[:, 2]).abs() > 1.3 * cam["tany"])

