"""The sweep voxel map (csrc/voxel.hip, include/gsraster.h gsr_voxel_sweep): a persistent voxel table on the device
with exact, order-independent per-voxel moments, and one oriented Gaussian per voxel that matures, registered under its
voxel key.  The step between admit_sweep (which points, which colour) and GrowableGaussians.add_new_pointcloud;
GrowableGaussians.add_voxel_seeds appends what `sweep` returns."""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _capi

# status codes of VoxelSeeds.status; VoxelSeeds.counts = (accumulated, seeded, out, full, matured, live keys)
ACCUMULATED, SEEDED, OUT, FULL = range(4)


class VoxelSeeds(NamedTuple):
    """What SweepVoxelMap.sweep returns.  One row per voxel that matured in the call, in the order of first appearance:
    xyz [v,3] the mean, covs [v,3,3] symmetric, rgbs [v,3] (0..255; None without colours), keys [v] int64, points [v]
    int32 the count, scaling_raw [v,3] = log sqrt(lambda * scale_factor) with lambda descending, rotation [v,4]
    (w, x, y, z) with w >= 0, normal [v,3] the axis of the smallest eigenvalue.  Per point of the sweep: status [n]
    uint8 and point_keys [n] int64 (-1 for OUT).  counts: six host ints."""
    xyz: torch.Tensor
    covs: torch.Tensor
    rgbs: Optional[torch.Tensor]
    keys: torch.Tensor
    points: torch.Tensor
    scaling_raw: torch.Tensor
    rotation: torch.Tensor
    normal: torch.Tensor
    status: torch.Tensor
    point_keys: torch.Tensor
    counts: Tuple[int, ...]


class SweepVoxelMap:
    """The voxels of every sweep so far.  grid: the voxel edge; min_points: the count at which a voxel matures, seeds
    its Gaussian and closes; min_sigma: the smallest standard deviation along an axis of a seed.  None of the three has
    a default: they are the caller's policy.  capacity: slots of the table, a power of two; it doubles as needed."""

    def __init__(self, grid, min_points, min_sigma, capacity=1 << 16, device="cuda"):
        self.grid, self.min_points, self.min_sigma = float(grid), int(min_points), float(min_sigma)
        self.device = torch.device(device)
        self.table = _capi.voxel_table(capacity, self.device)
        self.live = 0

    @property
    def capacity(self):
        return int(self.table.size(0))

    def grow(self, capacity=None):
        """Moves every record into a zeroed table of `capacity` slots (default: twice as many): one launch."""
        new = _capi.voxel_table(2 * self.capacity if capacity is None else capacity, self.device)
        self.table = _capi.voxel_rehash(self.table, new)

    @torch.no_grad()
    def sweep(self, points, colors=None, scale_factor=1.0):
        """points: [n,3] f32 on the device (n <= 2^22); colors: [n,3] f32 in 0..255 (Admitted.rgbs) or None.  The table
        grows BEFORE the launch whenever live + n > capacity / 2, so no point is ever FULL.  ONE host wait: the read of
        the counts.  Returns `VoxelSeeds`."""
        pts = points.detach().contiguous()
        n = int(pts.size(0))
        while 2 * (self.live + n) > self.capacity:
            self.grow()
        out, counts = _capi.voxel_sweep(pts, None if colors is None else colors.detach().contiguous(), self.grid,
                                        self.min_points, self.min_sigma, scale_factor, self.table, self.live)
        counts = tuple(int(c) for c in counts.tolist())   # the one host wait
        v, self.live = counts[4], counts[5]
        return VoxelSeeds(out["xyz"][:v], out["covs"][:v].view(v, 3, 3), None if out["rgb"] is None else out["rgb"][:v],
                          out["keys"][:v], out["points"][:v], out["scaling"][:v], out["rotation"][:v],
                          out["normal"][:v], out["status"][:n], out["point_keys"][:n], counts)

    @staticmethod
    def loss_points(points, seeds, max_points=500):
        """{voxel key: [k,3] f32 CPU tensor} of the SEEDED points of the sweep `seeds` came from, at most max_points
        per voxel (the first ones): the dict VoxelIndex.select and GrowableGaussians.calc_simi_loss take."""
        sel = (seeds.status == SEEDED).nonzero().squeeze(1)
        keys = seeds.point_keys.index_select(0, sel).cpu()
        pts = points.detach().index_select(0, sel).cpu()
        order = torch.argsort(keys, stable=True)
        uniq, cnt = torch.unique_consecutive(keys[order], return_counts=True)
        out, at = {}, 0
        for k, c in zip(uniq.tolist(), cnt.tolist()):
            out[k] = pts[order[at:at + min(c, int(max_points))]].contiguous()
            at += c
        return out

    def state(self):
        """The table's records SORTED BY KEY, as CPU int64 tensors: keys [m], closed [m], count [m], s1 [m,3], s2 [m,6]
        (xx, xy, xz, yy, yz, zz), sc [m,3].  The only window on the table, for tests and checkpoints."""
        t = self.table.cpu()
        t = t[t[:, 0] != 0]
        t = t[torch.argsort(t[:, 0])]
        return dict(keys=t[:, 0], closed=t[:, 1], count=t[:, 2], s1=t[:, 3:6], s2=t[:, 6:12], sc=t[:, 12:15])
