"""The delta-depth term between a keyframe pair (csrc/delta.hip, gsr_delta_depth_loss) restated for the tests.

restatement()   the reference's ops, one for one, from cam_points on (src/gs/gaussian.cu:116-199 -- meshgrid :121-127,
                d_uv and inv_K :129-136, T_trans applied :163, K_ref and the division :165-169, depth_values :171, the
                normalisation by W-1 / H-1 :173-181, grid_sample(bilinear, zeros, align_corners=True) :187-194 -- and
                src/liw/lioOptimization.cpp:1783-1799: inv_depth (include/gs/gs/loss_utils.cuh:15-21), the two masks,
                lambda * mean|.|).  dtype is a parameter: float64 is the truth, float32 the yardstick.  Gradients with
                respect to the two depth images come from autograd.  The kernel only ever sees T_rel, so does this.
explicit()      a second float64 evaluation with explicit index arithmetic (no grid_sample) and the analytic gradient,
                plus everything the bars need.
bars()          the bound of the fused call's error against float64 per compared quantity, and the fragile sets.
CASES / reference(case)   the inputs of tests/test_gpu_delta.py and their references, evaluated once per process.

Bars.  eps = 2^-23.  The kernels see the matrices composed on the host in double and rounded once (A = R_rel inv_K_src,
M = K_ref A, n = K_ref t_rel); a composed entry is bounded by the product of the absolute matrices, so magnitudes are
carried stepwise: q_abs = |inv_K| (u, v, 1), r_abs = |R| q_abs, p_abs = |d| r_abs + |t|, N_abs = |K_ref| p_abs,
m_abs = |K_ref| r_abs.  Counting roundings in csrc/delta.hip:
  Z' = fma(d, r_z, t_z), r_z two fma and one entry rounding per term          dZ  = 6 eps p_abs.z   (5 counted)
  N_c likewise; X = N_x / N_z one division                                    dX  = 6 eps (N_abs.x + |X| N_abs.z) / |N_z| + eps |X|
  out: 1 - f, four weight products, one product and three fma                 dout = sum_k w_k dZ_k + |s_x| dX + |s_y| dY + 6 eps sum_k w_k |Z_k|
       (s_x, s_y: the bilinear slopes -- the first-order term the rounding of (X, Y) carries; large next to a hole)
  a = 1 / out, b = 1 / depth_ref                                              da = dout / out^2 + eps a,  db = eps b
  gap = |a - b|                                                               dgap = mask (da + db + eps gap)
  mean gap: f64 sums, one division, one conversion; L one product more        lambda mean(dgap) + 6 eps L  (+ 100 / (H W) per pixel whose
                                                                              out lies within dout of the clamp 0.01)
  dL/ddepth_ref = c g b^2 (c = lambda / (H W): one rounding; b, b^2, product) 6 eps |.|
  u = -g a^2                                                                  du = 2 a dout / out^2 + 4 eps |u|
  tap sums S_j = sum u_i w_ik, exact up to the fixed point                    dS_j = sum (w_ik du_i + |u_i| (dX_i + dY_i))
                                                                                     + N_j N Mx 2^-59   (N_j contributions, half a grid
                                                                                     step each: 2^-s < N Mx 2^-58, see delta.hip)
  s_x = fma(f_y, Z11 - Z01, (1 - f_y)(Z10 - Z00))                             ds_x = sum_k dZ_k + dY (|Z10 - Z00| + |Z11 - Z01|) + 4 eps sum_k |Z_k|
  dX/dd = fma(-X, m_z, m_x) / N_z                                             ddX = (6 eps (m_abs.x + |X| m_abs.z) + dX |m_z|) / |N_z|
                                                                                    + |dX/dd| 6 eps N_abs.z / |N_z| + 2 eps |dX/dd|
  T_j = u_j (s_x dX/dd + s_y dY/dd)                                           dT by the product rule + 3 eps |u| (|s_x dX/dd| + |s_y dY/dd|)
  dL/ddepth_src = c fma(r_z, S_j, T_j)                                        c (|r_z| dS_j + (5 eps r_abs.z + 3 eps |r_z|) sum |u_i| w_ik + dT_j)
                                                                              + 3 eps c (|r_z S_j| + |T_j|)
Every quantity is held to max(2 e_ref, its bar), e_ref = |float32 restatement - float64| (for a gradient image: the
largest e_ref of the pixel's 3 x 3 neighbourhood, so that one lucky zero does not set a bar).

Fragile pixels, removed from both sides (at most 1 % of a case's pixels, or the case fails):
  F1  X or Y within dX / dY of an integer, for a pixel whose cell touches the image: the slope of another cell; affects
      that pixel's own dL/ddepth_src only
  F2  |out - 0.01| within dout: a (and the gradient) jumps; removes the pixel and, from dL/ddepth_src, its four taps.
      depth_ref is an input and compares exactly on both sides: no band.
  F3  |a - b| within da + db with a != b: the sign; removes the pixel from both gradients and its four taps from
      dL/ddepth_src.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 2.0 ** -23
COORD_MAX = 2.0 ** 30
MIN_DEPTH = 0.01


def inv_depth(x):
    """include/gs/gs/loss_utils.cuh:15-21"""
    return torch.where(x <= MIN_DEPTH, torch.zeros_like(x), 1.0 / torch.where(x <= MIN_DEPTH, torch.ones_like(x), x))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def forward_ops(ds, a_s, dr, a_r, inv_K_src, K_ref, T_rel, lam):
    """The reference's ops on tensors of one dtype ([1,H,W] images, 3x3, 3x3, 4x4): (loss, mean gap, mask, out)."""
    dtype, dev = ds.dtype, ds.device
    H, W = ds.shape[1], ds.shape[2]
    mx = torch.arange(0, W, dtype=dtype, device=dev).repeat(H, 1)           # gaussian.cu:121
    my = torch.arange(0, H, dtype=dtype, device=dev).unsqueeze(1).repeat(1, W)   # :122
    pix = torch.stack([mx.flatten(), my.flatten()], 0)                      # :125
    ones = torch.ones(1, pix.shape[1], dtype=dtype, device=dev)
    hom = torch.cat([pix, ones], 0)                                         # :127
    d_uv = hom * ds.flatten()                                               # :133
    cam = torch.matmul(inv_K_src, d_uv)                                     # :135
    cam = torch.cat([cam, ones], 0)                                         # :136
    proj = torch.matmul(T_rel, cam)                                         # :163
    p2 = torch.matmul(K_ref, proj[:3])                                      # :168
    pc = p2[:2] / p2[2].unsqueeze(0)                                        # :169
    zv = proj[2]                                                            # :171
    pc = pc.view(2, H, W).permute(1, 2, 0)                                  # :173
    gx = pc[:, :, 0] / (W - 1) * 2 - 1                                      # :176-178
    gy = pc[:, :, 1] / (H - 1) * 2 - 1                                      # :179-181
    grid = torch.stack([gx, gy], -1).unsqueeze(0)
    out = F.grid_sample(zv.view(1, 1, H, W), grid, mode="bilinear", padding_mode="zeros", align_corners=True)  # :187-194
    out = out.squeeze(0)                                                    # [1, H, W]
    a, b = inv_depth(out), inv_depth(dr)                                    # lioOptimization.cpp:1783-1784
    ms = torch.ones_like(a_s).masked_fill(a_s < 0.5, 0)                     # :1786-1788
    mr = torch.ones_like(a_r).masked_fill(a_r < 0.5, 0)                     # :1790-1792
    gap = torch.abs(a * ms * mr - b * mr * ms)                              # :1794-1797
    mean_gap = gap.mean()
    return lam * mean_gap, mean_gap, ms * mr, out                           # :1799


def restatement(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, lam, dtype=F64):
    """{loss, mean_gap, share, warped, grad_src, grad_ref} (module docstring).  T_rel: 3x4 or 4x4."""
    ds = _t(depth_src, dtype).reshape(1, *np.asarray(depth_src).shape[-2:]).clone().requires_grad_(True)
    dr = _t(depth_ref, dtype).reshape(ds.shape).clone().requires_grad_(True)
    a_s, a_r = _t(acc_src, dtype).reshape(ds.shape), _t(acc_ref, dtype).reshape(ds.shape)
    H, W = ds.shape[1], ds.shape[2]
    T = torch.eye(4, dtype=dtype)
    T[:3] = _t(T_rel, dtype).reshape(-1, 4)[:3]
    loss, mean_gap, mask, out = forward_ops(ds, a_s, dr, a_r, _t(inv_K_src, dtype).reshape(3, 3),
                                            _t(K_ref, dtype).reshape(3, 3), T, lam)
    g_s, g_r = torch.autograd.grad(loss, [ds, dr], allow_unused=True)
    z = lambda g: (torch.zeros_like(ds) if g is None else g).detach().reshape(H, W)  # noqa: E731
    return dict(loss=loss.detach(), mean_gap=mean_gap.detach(), share=mask.mean(), warped=out.detach().reshape(H, W),
                grad_src=z(g_s), grad_ref=z(g_r))


def explicit(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, lam):
    """Float64, index arithmetic only; returns the quantities of restatement() and the intermediates bars() needs."""
    ds = _t(depth_src, F64).reshape(-1)
    H, W = np.asarray(depth_src).shape[-2:]
    N = H * W
    dr, a_s, a_r = (_t(x, F64).reshape(-1) for x in (depth_ref, acc_src, acc_ref))
    iK, K = _t(inv_K_src, F64).reshape(3, 3), _t(K_ref, F64).reshape(3, 3)
    T = _t(T_rel, F64).reshape(-1, 4)[:3]
    R, t = T[:, :3], T[:, 3]
    idx = torch.arange(N)
    hom = torch.stack([(idx % W).to(F64), (idx // W).to(F64), torch.ones(N, dtype=F64)], 0)
    q = iK @ hom
    r = R @ q
    p = ds * r + t[:, None]
    Nn = K @ p
    m = K @ r
    zp = p[2]
    with np.errstate(all="ignore"):
        X, Y = Nn[0] / Nn[2], Nn[1] / Nn[2]
    fin = torch.isfinite(X) & torch.isfinite(Y) & (X.abs() <= COORD_MAX) & (Y.abs() <= COORD_MAX)
    Xs, Ys = torch.where(fin, X, torch.zeros_like(X)), torch.where(fin, Y, torch.zeros_like(Y))
    x0, y0 = torch.floor(Xs), torch.floor(Ys)
    fx, fy = Xs - x0, Ys - y0
    ix, iy = x0.long(), y0.long()
    inside = fin & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
    w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    ok, tap, z = [], [], []
    for k in range(4):
        xk, yk = ix + (k & 1), iy + (k >> 1)
        o = inside & (xk >= 0) & (xk < W) & (yk >= 0) & (yk < H)
        j = torch.where(o, yk * W + xk, torch.zeros_like(xk))
        ok.append(o); tap.append(j); z.append(torch.where(o, zp[j], torch.zeros_like(zp)))
    out = w[0] * z[0] + w[1] * z[1] + w[2] * z[2] + w[3] * z[3]
    out = torch.where(inside, out, torch.zeros_like(out))
    sx = torch.where(inside, (1 - fy) * (z[1] - z[0]) + fy * (z[3] - z[2]), torch.zeros_like(out))
    sy = torch.where(inside, (1 - fx) * (z[2] - z[0]) + fx * (z[3] - z[1]), torch.zeros_like(out))
    a, b = inv_depth(out), inv_depth(dr)
    on = (~(a_s < 0.5) & ~(a_r < 0.5)).to(F64)
    g = on * torch.sign(a - b)
    gap = on * (a - b).abs()
    mean_gap = gap.sum() / N
    c = lam / N
    grad_ref = torch.where(dr > MIN_DEPTH, c * g * b * b, torch.zeros_like(b))
    u = torch.where(out > MIN_DEPTH, -g * a * a, torch.zeros_like(a))
    dX = torch.where(inside, (m[0] - Xs * m[2]) / Nn[2], torch.zeros_like(X))
    dY = torch.where(inside, (m[1] - Ys * m[2]) / Nn[2], torch.zeros_like(X))
    S = torch.zeros(N, dtype=F64)
    for k in range(4):
        S.index_add_(0, tap[k][ok[k]], (u * w[k])[ok[k]])
    Tc = torch.where(u != 0, u * (sx * dX + sy * dY), torch.zeros_like(u))
    grad_src = c * (r[2] * S + Tc)
    return dict(loss=lam * mean_gap, mean_gap=mean_gap, share=on.mean(), warped=out.reshape(H, W),
                grad_src=grad_src.reshape(H, W), grad_ref=grad_ref.reshape(H, W),
                H=H, W=W, X=X, Y=Y, Xs=Xs, Ys=Ys, inside=inside, w=w, ok=ok, tap=tap, z=z, sx=sx, sy=sy, a=a, b=b,
                on=on, g=g, gap=gap, u=u, dX=dX, dY=dY, S=S, Tc=Tc, rz=r[2], Nn=Nn, m=m, c=c, lam=lam, ds=ds,
                hom=hom, iK=iK, K=K, R=R, t=t)


def bars(e):
    """Bars and fragile sets of one explicit() evaluation (module docstring): {'bar': {name: tensor}, 'F1','F2','F3':
    bool [N], 'taps_of': fn(mask) -> bool [N] (the pixels the masked pixels tap)}."""
    H, W = e["H"], e["W"]
    N = H * W
    q_abs = e["iK"].abs() @ e["hom"]
    r_abs = e["R"].abs() @ q_abs
    p_abs = e["ds"].abs() * r_abs + e["t"].abs()[:, None]
    N_abs = e["K"].abs() @ p_abs
    m_abs = e["K"].abs() @ r_abs
    Nz = e["Nn"][2].abs().clamp_min(1e-300)
    ins = e["inside"]
    zero = torch.zeros(N, dtype=F64)
    X, Y = e["Xs"].abs(), e["Ys"].abs()
    dZ = 6 * EPS * p_abs[2]
    dXc = torch.where(ins, 6 * EPS * (N_abs[0] + X * N_abs[2]) / Nz + EPS * X, zero)
    dYc = torch.where(ins, 6 * EPS * (N_abs[1] + Y * N_abs[2]) / Nz + EPS * Y, zero)
    w, ok, tap, z = e["w"], e["ok"], e["tap"], e["z"]
    dZk = [torch.where(ok[k], dZ[tap[k]], zero) for k in range(4)]
    sumz = sum(w[k] * z[k].abs() for k in range(4))
    dout = sum(w[k] * dZk[k] for k in range(4)) + e["sx"].abs() * dXc + e["sy"].abs() * dYc + 6 * EPS * sumz
    dout = torch.where(ins, dout, zero)
    out = e["warped"].reshape(-1)
    live = out > MIN_DEPTH
    safe = torch.where(live, out, torch.ones_like(out))
    da = torch.where(live, dout / (safe * safe), zero) + EPS * e["a"]
    db = EPS * e["b"]
    dgap = e["on"] * (da + db + EPS * e["gap"])
    F2 = ins & ((out - MIN_DEPTH).abs() <= dout)
    F3 = (e["on"] > 0) & (e["a"] != e["b"]) & ((e["a"] - e["b"]).abs() <= da + db)
    fr = lambda v: (v - torch.round(v)).abs()  # noqa: E731
    F1 = ins & ((fr(e["Xs"]) <= dXc) | (fr(e["Ys"]) <= dYc))
    lam, c = e["lam"], e["c"]
    bar_mean = dgap.sum() / N + 6 * EPS * e["mean_gap"] + 100.0 * float(F2.sum()) / N
    bar = dict(warped=dout.reshape(H, W), mean_gap=bar_mean, loss=lam * bar_mean + 6 * EPS * abs(lam) * e["mean_gap"],
               share=2 * EPS * e["share"], grad_ref=(6 * EPS * e["grad_ref"].abs()))
    u = e["u"].abs()
    du = torch.where(live, 2 * e["a"] * dout / (safe * safe), zero) + 4 * EPS * u
    Mx = float(u.max())
    dS, Sabs, cnt = torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
    for k in range(4):
        sel = ok[k] & (u > 0)
        dS.index_add_(0, tap[k][sel], (w[k] * du + u * (dXc + dYc))[sel])
        Sabs.index_add_(0, tap[k][sel], (w[k] * u)[sel])
        cnt.index_add_(0, tap[k][sel], torch.ones(N, dtype=F64)[sel])
    dS = dS + cnt * N * Mx * 2.0 ** -59
    sumzk = sum(z[k].abs() for k in range(4))
    sumdZ = sum(dZk)
    dsx = sumdZ + dYc * ((z[1] - z[0]).abs() + (z[3] - z[2]).abs()) + 4 * EPS * sumzk
    dsy = sumdZ + dXc * ((z[2] - z[0]).abs() + (z[3] - z[1]).abs()) + 4 * EPS * sumzk
    dXd, dYd = e["dX"].abs(), e["dY"].abs()
    mz = e["m"][2].abs()
    ddX = (6 * EPS * (m_abs[0] + X * m_abs[2]) + dXc * mz) / Nz + dXd * 6 * EPS * N_abs[2] / Nz + 2 * EPS * dXd
    ddY = (6 * EPS * (m_abs[1] + Y * m_abs[2]) + dYc * mz) / Nz + dYd * 6 * EPS * N_abs[2] / Nz + 2 * EPS * dYd
    sx, sy = e["sx"].abs(), e["sy"].abs()
    dT = du * (e["sx"] * e["dX"] + e["sy"] * e["dY"]).abs() + u * (dsx * dXd + sx * ddX + dsy * dYd + sy * ddY) \
        + 3 * EPS * u * (sx * dXd + sy * dYd)
    dT = torch.where(ins & (u > 0), dT, zero)
    rz = e["rz"].abs()
    gs = abs(c) * (rz * dS + (5 * EPS * r_abs[2] + 3 * EPS * rz) * Sabs + dT) \
        + 3 * EPS * abs(c) * ((e["rz"] * e["S"]).abs() + e["Tc"].abs())
    bar["grad_src"] = gs.reshape(H, W)

    def taps_of(mask):
        hit = torch.zeros(N, dtype=torch.bool)
        for k in range(4):
            hit[tap[k][ok[k] & mask]] = True
        return hit
    return dict(bar=bar, F1=F1, F2=F2, F3=F3, taps_of=taps_of, dXc=dXc, dYc=dYc)


def pool3(x):
    """largest value of each pixel's 3 x 3 neighbourhood"""
    return F.max_pool2d(x[None, None], 3, stride=1, padding=1)[0, 0]


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------
def _rot(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = (f(math.radians(v)) for v in (roll, pitch, yaw) for f in (math.cos, math.sin))
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Rz @ Rx @ Ry


POSES = {   # (roll, pitch, yaw in degrees about z, x, y of the camera; t_rel in metres)
    "small": ((0.0, 0.0, 1.3), (0.06, 0.0, 0.015)),             # 1.3 degrees of yaw and 6 cm; the holes leave the image
    "rpy": ((2.0, -1.5, 2.5), (0.02, -0.01, 0.05)),             # every entry of R_rel non-zero; the holes all land in ONE cell inside
    "shift": ((0.0, 0.0, 18.0), (0.1, 0.0, 0.02)),              # about 30 % of the samples leave the image
    "backward": ((0.5, 0.4, -1.0), (0.02, 0.01, -3.5)),         # p'.z <= 0 for the near part of the scene
}
CASES = (("2x2", 2, 2, "small", 1), ("5x3", 5, 3, "rpy", 2), ("37x61_small", 37, 61, "small", 3),
         ("37x61_rpy", 37, 61, "rpy", 4), ("37x61_shift", 37, 61, "shift", 5), ("37x61_backward", 37, 61, "backward", 6),
         ("64x80_small", 64, 80, "small", 7), ("64x80_shift", 64, 80, "shift", 8), ("70x130_rpy", 70, 130, "rpy", 9),
         ("70x130_backward", 70, 130, "backward", 10), ("512x640_small", 512, 640, "small", 11))
CASE_NAMES = tuple(c[0] for c in CASES)
LAMBDA = 0.2


def intrinsics(H, W):
    """K_src, K_ref (fx != fy, principal points off centre, K_src != K_ref) and inv(K_src), float32."""
    Ks = np.array([[0.9 * W, 0, W / 2 + 1.3], [0, 1.07 * W, H / 2 - 0.7], [0, 0, 1]], np.float64)
    Kr = np.array([[0.93 * W, 0, W / 2 + 2.2], [0, 1.04 * W, H / 2 - 0.3], [0, 0, 1]], np.float64)
    return Ks.astype(np.float32), Kr.astype(np.float32), np.linalg.inv(Ks).astype(np.float32)


def pose(name):
    (roll, pitch, yaw), t = POSES[name]
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = _rot(roll, pitch, yaw), t
    return T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The float32 inputs of one of CASES: smooth depth of 2-8 m plus noise; depth_ref = depth_src -+ an offset per
    8 x 8 block; silhouettes in [0.7, 1] with one rectangle below 0.5 on each side; a rectangle of holes (depth exactly 0)
    in src, half of it under the src mask; ref depths of 0.005 and of exactly 0.01 in unmasked pixels."""
    name, H, W, pname, seed = next(c for c in CASES if c[0] == case)
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    ds = 5.0 + 2.4 * np.sin(0.11 * u + 0.3 * seed) * np.cos(0.09 * v + 0.2) + 0.5 * np.sin(0.031 * (u + v))
    ds = ds + rng.uniform(-0.02, 0.02, (H, W))
    blk = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8)) * 2 - 1
    off = rng.uniform(0.15, 0.4, (H, W)) * np.kron(blk, np.ones((8, 8)))[:H, :W]
    dr = ds + off
    a_s, a_r = rng.uniform(0.7, 1.0, (H, W)), rng.uniform(0.7, 1.0, (H, W))
    if H >= 16 and W >= 16:
        a_s[H // 5:H // 5 + H // 4, W // 6:W // 6 + W // 4] = rng.uniform(0.05, 0.45, (H // 4, W // 4))
        a_r[H // 2:H // 2 + H // 5, W // 2:W // 2 + W // 3] = rng.uniform(0.05, 0.45, (H // 5, W // 3))
        ds[H // 5 + H // 8:H // 5 + H // 4 + H // 8, W // 6 + 2:W // 6 + W // 4 - 2] = 0.0     # holes
        dr[3 * H // 4:3 * H // 4 + 3, W // 8:W // 8 + 5] = 0.005
        dr[3 * H // 4 + 4, W // 8:W // 8 + 5] = np.float32(0.01)
        dr[H // 2 + 1:H // 2 + 3, W // 2 + 1:W // 2 + 4] = 0.0                                  # (and under the ref mask)
    elif H * W >= 15:
        ds[1, 1] = 0.0
        dr[2, 1] = 0.005
        a_s[0, 2] = 0.3
        a_r[3, 0] = 0.2
    Ks, Kr, iKs = intrinsics(H, W)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(depth_src=f(ds), acc_src=f(a_s), depth_ref=f(dr), acc_ref=f(a_r), inv_K_src=iKs, K_ref=Kr,
                T_rel=pose(pname), lam=LAMBDA, H=H, W=W)


def _args(x):
    return (x["depth_src"], x["acc_src"], x["depth_ref"], x["acc_ref"], x["inv_K_src"], x["K_ref"], x["T_rel"], x["lam"])


def evaluate(x):
    """float64 truth (explicit), float32 yardstick (restatement) and the final bars / keep masks of one input set."""
    e = explicit(*_args(x))
    y32 = restatement(*_args(x), dtype=torch.float32)
    b = bars(e)
    H, W = e["H"], e["W"]
    bar, keep, eref = {}, {}, {}
    for k in ("warped", "grad_src", "grad_ref"):
        er = (y32[k].to(F64) - e[k]).abs()
        er = torch.where(torch.isfinite(er), er, torch.zeros_like(er))
        eref[k] = er if k == "warped" else pool3(er)
        bar[k] = torch.maximum(2 * eref[k], b["bar"][k])
    for k in ("loss", "mean_gap", "share"):
        eref[k] = (y32[k].to(F64) - e[k]).abs()
        bar[k] = torch.maximum(2 * eref[k], torch.as_tensor(b["bar"][k], dtype=F64))
    F1, F2, F3 = b["F1"], b["F2"], b["F3"]
    t23 = b["taps_of"](F2 | F3)
    keep["warped"] = (~F2).reshape(H, W)
    keep["grad_ref"] = (~(F2 | F3)).reshape(H, W)
    keep["grad_src"] = (~(F1 | F2 | F3 | t23)).reshape(H, W)
    share = float((F1 | F2 | F3).to(F64).mean())
    return dict(truth=e, f32=y32, bar=bar, keep=keep, fragile_share=share, eref=eref)


@functools.lru_cache(maxsize=None)
def reference(case):
    return evaluate(inputs(case))


def ratios(got, ref):
    """worst |got - truth| / bar per quantity over the kept pixels; got: {name: float64 tensor}."""
    out = {}
    for k in ("warped", "grad_src", "grad_ref"):
        d = (got[k].to(F64) - ref["truth"][k]).abs() / ref["bar"][k].clamp_min(1e-300)
        d = torch.where(ref["keep"][k], d, torch.zeros_like(d))
        zero_bar = ref["keep"][k] & (ref["bar"][k] == 0)          # a bar of 0 demands equality
        d = torch.where(zero_bar, (got[k].to(F64) != ref["truth"][k]).to(F64) * 1e9, d)
        out[k] = float(d.max())
    for k in ("loss", "mean_gap", "share"):
        diff, bar = abs(float(got[k]) - float(ref["truth"][k])), float(ref["bar"][k])
        out[k] = diff / bar if bar > 0 else (0.0 if diff == 0 else 1e9)
    return out
