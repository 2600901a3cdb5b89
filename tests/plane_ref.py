"""Restatement of the point-to-plane LiDAR loss on oriented surfels (include/gsraster.h, gsr_surfel_plane_loss) in
plain PyTorch ops, the scenes its tests run on, and the analysis both test files share.

    k*_j = argmin_k scaling[sel_j][k]               (the first minimal index on a tie)
    n_j  = column k*_j of R(rotation[sel_j])        R: the polynomial of (w, x, y, z), not renormalised
    j(i) = argmin_j |p_i - xyz[sel_j]|^2            (the first minimal position on a tie)
    v_i  = p_i - xyz[sel_j(i)],  d_i = |v_i|,  g_i = [d_i <= max_dist],  e_i = n_j(i) . v_i
    loss = lambda / m * sum_i g_i rho(e_i) + lambda_flat / n * sum_j scaling[sel_j][k*_j]

`plane_loss_ref` is that, in whatever dtype the inputs have, with the gradients left to autograd: in float64 it is the
truth, in float32 the yardstick (tests/test_gpu_plane.py).  `plane_loss_closed` writes the gradients out (A_j, B_j and
the 3x4 Jacobian of the column) without autograd, so that a MUTANT can be planted in any line of forward or backward;
unmutated it equals autograd (tests/test_plane_ref.py).
"""
import numpy as np
import torch

import simi_ref

# (m, n) -> selected voxels, Gaussians per voxel of simi_ref.make_scene
CASES = {(1, 1): (1, 1), (7, 16): (1, 16), (65, 272): (17, 16), (2500, 16): (1, 16), (500, 8000): (500, 16)}
LAM = 0.2
# (huber, max_dist, lambda_flat)
PARAMS = [(0.0, float("inf"), 0.0), (0.02, 0.05, 0.3), (0.02, 0.08, 0.0)]
MUTANTS = ("largest_scale_column", "transposed_R", "sign_dropped_from_B", "gate_on_d2", "huber_slope_halved",
           "w_gradient_dropped")


def rotation_matrix(q):
    """R(q) [.., 3, 3] of q = (w, x, y, z) [.., 4], as given (no normalisation)."""
    w, x, y, z = q.unbind(-1)
    rows = [torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
            torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
            torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)]
    return torch.stack(rows, -2)


def nearest(points, centres, block=256):
    """Position of the nearest centre per point: broadcasting in blocks of points (no cdist: nothing here should depend
    on a library's choice of algorithm at a given size)."""
    out = []
    c = centres.detach()
    for lo in range(0, points.shape[0], block):
        diff = points[lo:lo + block, None, :].detach() - c[None, :, :]
        out.append((diff * diff).sum(2).argmin(1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.long, device=points.device)


def rho(e, huber):
    if huber > 0:
        return torch.where(e.abs() <= huber, e * e / (2 * huber), e.abs() - huber / 2)
    return e.abs()


def plane_parts_ref(points, sel, xyz, scaling, rotation, lambda_, huber=0.0, max_dist=float("inf"), lambda_flat=0.0):
    """out4 = [loss, mean gated rho, mean thinnest scale, share of points inside max_dist] as a list of 0-dim tensors
    (the first three differentiable)."""
    idx = sel.long()
    x, s, q = xyz.index_select(0, idx), scaling.index_select(0, idx), rotation.index_select(0, idx)
    m, n = points.shape[0], idx.shape[0]
    ks = s.argmin(1)
    normal = rotation_matrix(q).gather(2, ks[:, None, None].expand(n, 3, 1)).squeeze(2)   # column k* of every R
    thin = s.gather(1, ks[:, None]).squeeze(1)
    j = nearest(points, x)
    v = points - x.index_select(0, j)
    gate = (v.detach().norm(2, 1) <= max_dist).to(points.dtype)
    e = (normal.index_select(0, j) * v).sum(1)
    mean_rho = (gate * rho(e, huber)).sum() / m
    mean_thin = thin.sum() / n
    return [lambda_ * mean_rho + lambda_flat * mean_thin, mean_rho, mean_thin, gate.sum() / m]


def plane_loss_ref(points, sel, xyz, scaling, rotation, lambda_, huber=0.0, max_dist=float("inf"), lambda_flat=0.0):
    return plane_parts_ref(points, sel, xyz, scaling, rotation, lambda_, huber, max_dist, lambda_flat)[0]


def reference(points, sel, xyz, scaling, rotation, params, dtype, lambda_=LAM):
    """The restatement in `dtype` with autograd: dict of out4 [4] and the dense gradients gx, gs [P,3], gr [P,4], all
    returned as float64."""
    huber, max_dist, lambda_flat = params
    # (fresh leaves: .to() of a tensor that already has the dtype is the tensor itself)
    x, s, q = (t.detach().to(dtype).clone().requires_grad_(True) for t in (xyz, scaling, rotation))
    parts = plane_parts_ref(points.to(dtype), sel, x, s, q, lambda_, huber, max_dist, lambda_flat)
    gx, gs, gr = torch.autograd.grad(parts[0], (x, s, q), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t).double() if g is None else g.double()
    return dict(out4=torch.stack([p.detach().double() for p in parts]), gx=z(gx, x), gs=z(gs, s), gr=z(gr, q))


def column_jacobian_T(ks, q, b):
    """(dn/dq)^T b per row: n = column ks of R(q); q [n,4], b [n,3] -> [n,4] (w, x, y, z)."""
    w, x, y, z = q.unbind(-1)
    b0, b1, b2 = b.unbind(-1)
    c0 = torch.stack([2 * (z * b1 - y * b2), 2 * (y * b1 + z * b2), -4 * y * b0 + 2 * x * b1 - 2 * w * b2,
                      -4 * z * b0 + 2 * w * b1 + 2 * x * b2], -1)
    c1 = torch.stack([2 * (x * b2 - z * b0), 2 * y * b0 - 4 * x * b1 + 2 * w * b2, 2 * (x * b0 + z * b2),
                      -2 * w * b0 - 4 * z * b1 + 2 * y * b2], -1)
    c2 = torch.stack([2 * (y * b0 - x * b1), 2 * z * b0 - 2 * w * b1 - 4 * x * b2, 2 * w * b0 + 2 * z * b1 - 4 * y * b2,
                      2 * (x * b0 + y * b1)], -1)
    return torch.where((ks == 0)[:, None], c0, torch.where((ks == 1)[:, None], c1, c2))


@torch.no_grad()
def plane_loss_closed(points, sel, xyz, scaling, rotation, params, lambda_=LAM, mutant=None):
    """The term with its gradients written out (no autograd); `mutant` (one of MUTANTS) plants one wrong line.
    Same dict as `reference`, in float64 whatever the dtype of the arithmetic."""
    assert mutant is None or mutant in MUTANTS
    huber, max_dist, lambda_flat = params
    idx = sel.long()
    x, s, q = xyz.index_select(0, idx), scaling.index_select(0, idx), rotation.index_select(0, idx)
    m, n, P = points.shape[0], idx.shape[0], xyz.shape[0]
    ks = s.argmax(1) if mutant == "largest_scale_column" else s.argmin(1)
    R = rotation_matrix(q)
    if mutant == "transposed_R":
        R = R.transpose(1, 2)
    normal = R.gather(2, ks[:, None, None].expand(n, 3, 1)).squeeze(2)
    thin = s.gather(1, ks[:, None]).squeeze(1)
    j = nearest(points, x)
    v = points - x.index_select(0, j)
    d = v.norm(2, 1)
    gate = ((d * d if mutant == "gate_on_d2" else d) <= max_dist).to(points.dtype)
    e = (normal.index_select(0, j) * v).sum(1)
    if huber > 0:
        slope = e / (2 * huber if mutant == "huber_slope_halved" else huber)
        drho = torch.where(e.abs() <= huber, slope, torch.sign(e))
    else:
        drho = torch.sign(e)
    mean_rho = (gate * rho(e, huber)).sum() / m
    mean_thin = thin.sum() / n
    out4 = torch.stack([lambda_ * mean_rho + lambda_flat * mean_thin, mean_rho, mean_thin, gate.sum() / m])
    A = torch.zeros(n, dtype=points.dtype, device=points.device).index_add_(0, j, gate * drho)
    wB = drho.abs() if mutant == "sign_dropped_from_B" else drho
    B = torch.zeros((n, 3), dtype=points.dtype, device=points.device).index_add_(0, j, (gate * wB)[:, None] * v)
    c = lambda_ / m
    gq = column_jacobian_T(ks, q, c * B)
    if mutant == "w_gradient_dropped":
        gq[:, 0] = 0
    gx, gs, gr = torch.zeros_like(xyz), torch.zeros_like(scaling), torch.zeros_like(rotation)
    gx[idx] = -(c * A)[:, None] * normal
    gr[idx] = gq
    gs[idx] = torch.nn.functional.one_hot(ks, 3).to(points.dtype) * (lambda_flat / n)
    return dict(out4=out4.double(), gx=gx.double(), gs=gs.double(), gr=gr.double())


@torch.no_grad()
def analyse(points, sel, xyz, scaling, rotation, params):
    """float64 facts per point (winner j, v, d, e, gate, rho', the magnitude E the roundings of e scale with) and which
    points are FRAGILE -- a float32 evaluation may put them on the other side of a comparison:
      * the two nearest centres differ by less than 1e-5 relative;
      * |e| < 1e-5 d with huber = 0 (with huber > 0, rho is quadratic at e = 0: a sign flip there changes no output);
      * |d - max_dist| < 1e-5 max_dist;
      * the winner's two smallest scales differ by less than 1e-5 relative."""
    huber, max_dist, _ = params
    idx = sel.long()
    x, s, q = xyz.double().index_select(0, idx), scaling.double().index_select(0, idx), rotation.double().index_select(0, idx)
    p = points.double()
    n = idx.shape[0]
    j, d1, d2 = [], [], []
    for lo in range(0, p.shape[0], 256):
        dd = (p[lo:lo + 256, None, :] - x[None, :, :]).norm(2, 2)
        best, arg = dd.min(1)
        j.append(arg)
        d1.append(best)
        if n > 1:
            dd.scatter_(1, arg[:, None], float("inf"))
            d2.append(dd.min(1).values)
    j, d = torch.cat(j), torch.cat(d1)
    ks = s.argmin(1)
    normal = rotation_matrix(q).gather(2, ks[:, None, None].expand(n, 3, 1)).squeeze(2)
    v = p - x.index_select(0, j)
    e = (normal.index_select(0, j) * v).sum(1)
    fragile = torch.zeros_like(d, dtype=torch.bool)
    if n > 1:
        fragile |= (torch.cat(d2) - d) < 1e-5 * d
    if huber == 0:
        fragile |= e.abs() < 1e-5 * d
    if max_dist < float("inf"):
        fragile |= (d - max_dist).abs() < 1e-5 * max_dist
    two = s.sort(1).values[:, :2]
    fragile |= ((two[:, 1] - two[:, 0]) < 1e-5 * two[:, 1]).index_select(0, j)
    gate = d <= max_dist
    drho = torch.where(e.abs() <= huber, e / huber, torch.sign(e)) if huber > 0 else torch.sign(e)
    knee = (e.abs() <= huber) if huber > 0 else torch.zeros_like(gate)
    N = 1 + 2 * (q * q).sum(1)                       # bounds the sum of the absolute monomials of any entry of R(q)
    v1 = v.abs().sum(1)
    E = N.index_select(0, j) * v1                    # what the absolute rounding error of e = n . v scales with
    return dict(j=j, d=d, e=e, v1=v1, gate=gate, drho=drho, knee=knee, E=E, N=N, q=q, ks=ks, fragile=fragile,
                rho=rho(e, huber))


def make_scene(n_selected_voxels, m, seed, **kw):
    """simi_ref.make_scene plus what makes its Gaussians surfels: `rotation` [P,4] float32, random unit quaternions
    with w >= 0, and per row one randomly chosen axis of `scaling` thinned to 0.2-0.5 of the row's smallest scale."""
    sc = simi_ref.make_scene(n_selected_voxels, m, seed, **kw)
    rng = np.random.default_rng(seed + 77)
    P = sc["P"]
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1
    scaling = sc["scaling"].astype(np.float64)
    axis = rng.integers(0, 3, P)
    scaling[np.arange(P), axis] = scaling.min(1) * rng.uniform(0.2, 0.5, P)
    sc["scaling"] = scaling.astype(np.float32)
    sc["rotation"] = q.astype(np.float32)
    return sc


def case_inputs(m, n, device="cpu"):
    """The inputs of GPU case (m, n), before any fragile point is removed: the scene, the selection VoxelIndex.select
    makes of it, and the model arrays as tensors on `device`."""
    import gs_livm_amd as G
    voxels, per = CASES[(m, n)]
    sc = make_scene(voxels, m, seed=1000 + n + m, per_voxel=per, empty_voxels=0 if voxels == 1 else 3)
    vi = G.VoxelIndex(torch.device("cpu"))
    vi.add(sc["keys"], sc["counts"], 0)
    points, sel = vi.select(sc["losses"], max_points=10 ** 9)
    assert points.shape == (m, 3) and sel.shape == (n,) and sc["P"] >= (4 * n if n > 16 else n)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return dict(scene=sc, P=sc["P"], points=points.to(device), sel=sel.to(device), xyz=t(sc["xyz"]),
                scaling=t(sc["scaling"]), rotation=t(sc["rotation"]))
