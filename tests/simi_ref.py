"""Restatement of GS-LIVM's LiDAR similarity loss in plain PyTorch ops, and the scenes its tests run on.

The loss (GaussianModel::compute_min_distance, src/gs/gaussian.cu:87-114) and the selection that feeds it
(calcSimiLoss, :201-228) are written here from their definition:

    r      = mean(scales)                     one scalar over all 3n selected elements
    d_ij   = || p_i - x_j ||_2                an [m, n] matrix
    loss   = lambda * mean_i min_j max(d_ij - r, 0)

in whatever dtype the inputs have.  Run in float64 it is the yardstick of the HIP kernels (gradients from autograd, as
tests/ref64.py does for the rasterizer); run in float32 it is the arithmetic the reference itself executes, and its
distance to the float64 result is the measure of what float32 can deliver (tests/test_gpu_simi.py).
"""
import numpy as np
import torch

VOXEL = 0.2          # metres
PER_VOXEL = 16       # Gaussians a voxel contributes: a jittered 4 x 4 patch of a plane


def compute_min_distance(points, centres, scales):
    """mean_i min_j max(||p_i - x_j|| - mean(scales), 0); points [m,3], centres [n,3], scales [n,3]."""
    r = scales.mean()
    m, n = points.shape[0], centres.shape[0]
    diff = points.unsqueeze(1).expand(m, n, 3) - centres.unsqueeze(0).expand(m, n, 3)
    dist = diff.norm(2, 2) - r
    clamped = torch.maximum(dist, torch.zeros_like(dist))
    return clamped.min(1).values.mean()


def similarity_loss_ref(points, sel, xyz, scaling, lambda_):
    """The term as calcSimiLoss assembles it (:219-237): rows `sel` of xyz / activated scaling, then the loss."""
    idx = sel.long()
    return lambda_ * compute_min_distance(points, xyz.index_select(0, idx), scaling.index_select(0, idx))


def select_by_mask(index, losses, P):
    """The selection of calcSimiLoss (:201-221) taken literally: `index` {key: list of rows}, `losses` {key: [k,3]
    tensor}.  Every key of `losses` that `index` knows appends its rows to a list and its points to a tensor; the
    rows are scattered into a mask over the P Gaussians and read back with nonzero().  Returns (points [m,3], rows
    [n] int64 ascending) or None when no point is left."""
    mask_indexes = []
    points = torch.empty((0, 3), dtype=torch.float32)
    for key, tensor in losses.items():
        if key in index:
            mask_indexes.extend(index[key])
            points = torch.cat([points, tensor.reshape(-1, 3).float()], 0)
    if points.shape[0] == 0:
        return None
    loss_mask = torch.zeros(P, dtype=torch.long)
    loss_mask.scatter_(0, torch.tensor(mask_indexes, dtype=torch.long), 1)
    return points, loss_mask.nonzero().squeeze(1)


TIE_CASES = [(64, 768, 64), (32768, 768, 192)]     # (m, n, D)
TIE_QUATERNIONS = ((1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, 0.25), (0.75, 0.25, -0.5, 0.5))


def tie_inputs(m, n, D, device="cpu"):
    """Inputs on which every point is at the SAME squared distance, bit for bit, from n / D selected centres: D
    distinct centres on the integer lattice 8 x 8 x (D / 64), position k of `sel` holding lattice point k mod D (P = 2n
    rows, the odd ones selected, so `sel` itself is unique), point i = lattice point i mod D + (1/8, 1/16, 0).
    Everything is dyadic: the squared distance to the own lattice point is 5/256 in any order of operations, with or
    without a fused multiply-add, and the next lattice point is 0.77 away.  All scales are 2^-6 (r = 2^-6 exactly: every
    point lies outside it; k* = 0 on every row); the quaternion of position k is entry (k + k // D) mod 4 of a dyadic
    table, so that the copies of a centre differ in their normals."""
    assert D % 64 == 0 and n % D == 0
    cell = torch.arange(D)
    lattice = torch.stack([cell % 8, (cell // 8) % 8, cell // 64], 1).float()
    k = torch.arange(n)
    P = 2 * n
    xyz = lattice[k % D].repeat_interleave(2, 0)
    rotation = torch.tensor(TIE_QUATERNIONS)[(k + k // D) % 4].repeat_interleave(2, 0)
    points = lattice[torch.arange(m) % D] + torch.tensor([0.125, 0.0625, 0.0])
    return dict(P=P, m=m, n=n, D=D, points=points.to(device), sel=(2 * k + 1).int().to(device),
                xyz=xyz.contiguous().to(device), scaling=torch.full((P, 3), 2.0 ** -6).to(device),
                rotation=rotation.contiguous().to(device))


def voxel_key(ix, iy, iz):
    """A distinct non-negative key per lattice cell (|i| < 2^15 per axis)."""
    return (int(ix) + 32768) | ((int(iy) + 32768) << 16) | ((int(iz) + 32768) << 32)


def make_scene(n_selected_voxels, m, seed, spare_voxels=None, empty_voxels=3, unknown_keys=4, per_voxel=PER_VOXEL,
               scale_median=0.02, scale_sigma=0.3):
    """A map of voxels with Gaussians on plane patches and LiDAR points in some of them.

    The model holds `n_selected_voxels + spare_voxels` voxels of VOXEL metres on a lattice, in shuffled order, each
    with `per_voxel` Gaussians on a jittered 4 x 4 patch of a tilted plane through the voxel (fewer than 16: the first
    ones of the patch) and log-normal activated scales around `scale_median`; `empty_voxels` more are registered
    without rows.  `m` LiDAR points lie uniformly inside the selected voxels (every selected voxel gets its share, the
    remainder goes to random ones; two of the m lie in an empty voxel when there is one and m allows it);
    `unknown_keys` further voxels carry three points each but are not in the model.

    Returns a dict: xyz, scaling [P,3] float32 numpy (scaling ACTIVATED), keys / counts (the model's voxels in row
    order, empty ones included), index {key: list of rows}, losses {key: [k,3] float32 CPU tensor} (unknown keys
    included, insertion order shuffled), n = rows selected, m = points under known keys.
    """
    rng = np.random.default_rng(seed)
    if spare_voxels is None:
        spare_voxels = 3 * n_selected_voxels + 5   # P is about four times the selection
    total = n_selected_voxels + spare_voxels + empty_voxels + unknown_keys
    side = int(np.ceil(total ** (1.0 / 3.0))) + 2
    cells = rng.permutation(side ** 3)[:total]
    coords = np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).astype(np.int64) - side // 2
    n_model = n_selected_voxels + spare_voxels
    model_cells, empty_cells = coords[:n_model], coords[n_model:n_model + empty_voxels]
    unknown_cells = coords[n_model + empty_voxels:]
    # Gaussians: a 4 x 4 grid in the plane's own (u, v), jittered, on a tilted plane through the voxel centre
    g = (np.arange(4) + 0.5) / 4.0 - 0.5
    uu, vv = np.meshgrid(g, g, indexing="ij")
    uv = np.stack([uu.ravel(), vv.ravel()], 1)[:per_voxel] if per_voxel <= 16 else None
    assert uv is not None, "at most 16 Gaussians per voxel"
    jit = rng.uniform(-0.3, 0.3, (n_model, per_voxel, 2)) / 4.0
    tilt = rng.uniform(-0.4, 0.4, (n_model, 2))
    off = rng.uniform(-0.25, 0.25, n_model)
    u = uv[None, :, 0] + jit[..., 0]
    v = uv[None, :, 1] + jit[..., 1]
    w = np.clip(off[:, None] + tilt[:, :1] * u + tilt[:, 1:] * v, -0.49, 0.49)
    local = np.stack([u, v, w], 2)                                  # [voxel, gaussian, (u, v, w)]
    perm = np.array([[2, 0, 1], [0, 2, 1], [0, 1, 2]])[rng.integers(0, 3, n_model)]  # the normal along x, y or z
    placed = np.take_along_axis(local, np.broadcast_to(perm[:, None, :], local.shape), 2)
    xyz = (model_cells[:, None, :] + 0.5 + placed) * VOXEL
    scaling = scale_median * np.exp(scale_sigma * rng.standard_normal((n_model, per_voxel, 3)))
    xyz = xyz.reshape(-1, 3).astype(np.float32)
    scaling = scaling.reshape(-1, 3).astype(np.float32)
    # the model's voxels in row order, the empty ones sprinkled between them
    keys, counts, index = [], [], {}
    empty_at = sorted(rng.integers(0, n_model + 1, empty_voxels).tolist())
    empties = [voxel_key(*c) for c in empty_cells]
    row = 0
    for v_i in range(n_model + 1):
        while empty_at and empty_at[0] == v_i:
            empty_at.pop(0)
            k = empties[len(empty_at)]
            keys.append(k); counts.append(0); index[k] = []
        if v_i == n_model:
            break
        k = voxel_key(*model_cells[v_i])
        keys.append(k); counts.append(per_voxel); index[k] = list(range(row, row + per_voxel))
        row += per_voxel
    # LiDAR points: uniform inside the selected voxels
    chosen = rng.permutation(n_model)[:n_selected_voxels]
    in_empty = 2 if empty_voxels and m >= n_selected_voxels + 2 else 0  # an empty voxel may receive points as well
    m_sel = m - in_empty
    per = np.full(n_selected_voxels, m_sel // n_selected_voxels, dtype=np.int64)
    np.add.at(per, rng.integers(0, n_selected_voxels, m_sel - int(per.sum())), 1)
    losses = {}
    for v_i, k_pts in zip(chosen, per):
        p = (model_cells[v_i][None, :] + rng.uniform(0, 1, (int(k_pts), 3))) * VOXEL
        losses[voxel_key(*model_cells[v_i])] = torch.from_numpy(p.astype(np.float32))
    for c in unknown_cells:  # keys the model does not know: their points must be dropped
        p = (c[None, :] + rng.uniform(0, 1, (3, 3))) * VOXEL
        losses[voxel_key(*c)] = torch.from_numpy(p.astype(np.float32))
    if in_empty:  # its key is known, it has no rows: the points stay, nothing is selected for them
        p = (empty_cells[0][None, :] + rng.uniform(0, 1, (in_empty, 3))) * VOXEL
        losses[voxel_key(*empty_cells[0])] = torch.from_numpy(p.astype(np.float32))
    order = rng.permutation(len(losses))
    items = list(losses.items())
    losses = {items[i][0]: items[i][1] for i in order}
    m_known = int(sum(v.shape[0] for k, v in losses.items() if k in index))
    return dict(xyz=xyz, scaling=scaling, keys=keys, counts=counts, index=index, losses=losses,
                n=n_selected_voxels * per_voxel, m=m_known, P=xyz.shape[0])
