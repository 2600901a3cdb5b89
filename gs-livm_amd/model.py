"""Host-side mirror of the pieces of GaussianModel that sit either side of the rasterizer, on the fused
kernels of csrc/optimizer.hip (SURVEY.md section 8(f) "next" row 1):

  * `FusedActivations` -- the getters Get_scaling / Get_rotation / Get_opacity / Get_features
    (include/gs/gs/gaussian.cuh:40-54) as ONE autograd node instead of five Torch ops;
  * `GaussianParameters` -- the six leaf tensors with those getter names;
  * `FusedAdam` -- torch::optim::Adam as the reference configures it (src/gs/gaussian.cu:396-428: one group
    per leaf, eps 1e-15, betas (0.9, 0.999), no weight decay) stepping every group in one launch and clearing
    the gradients it consumed (step + zero_grad, src/liw/lioOptimization.cpp:1831-1832);
  * `GrowableGaussians` -- row 4: the model as capacity buffers that grow in place
    (GaussianModel::addNewPointcloud / densification_postfix / cat_tensors_to_optimizer,
    src/gs/gaussian.cu:241-313, 451-472, 524-540);
  * `GrowableGaussians.prune` / `prune_rows` -- the shrinking half, GaussianModel::prune_optimizer (gaussian.cu:430-449,
    which the reference carries and never calls): rows that are dead to the rasterizer for good leave the leaves, the
    Adam moments and the voxel index by a stable compaction (csrc/prune.hip);
  * `GrowableGaussians.enable_density_stats` / `accumulate_density` / `densify` -- adaptive density control, upstream's
    clone and split (N = 2) of which the reference carries the remains (densification_postfix, gaussian.cu:521-540) and
    never runs: in place on the capacity buffers, existing rows keeping their numbers (csrc/densify.hip);
  * `VoxelIndex` -- gs_hash_indexes_ (voxel key -> rows of its Gaussians, gaussian.cu:257-263) and the selection
    of calcSimiLoss (:201-228) on row RANGES, which feeds the fused similarity loss (csrc/simi.hip, loss.py).
"""
import numpy as np
import torch

from . import _capi


class FusedActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling_raw, rotation_raw, opacity_raw, features_dc, features_rest):
        scales, rot, opac, shs = _capi.activate(scaling_raw.contiguous(), rotation_raw.contiguous(),
                                                opacity_raw.contiguous(), features_dc.contiguous(),
                                                features_rest.contiguous())
        ctx.save_for_backward(rotation_raw, scales, opac)
        return scales, rot, opac, shs

    @staticmethod
    def backward(ctx, g_scales, g_rot, g_opac, g_shs):
        rotation_raw, scales, opac = ctx.saved_tensors
        z = torch.zeros_like
        g_scales = z(scales) if g_scales is None else g_scales.contiguous()
        g_rot = z(rotation_raw) if g_rot is None else g_rot.contiguous()
        g_opac = z(opac) if g_opac is None else g_opac.contiguous()
        assert g_shs is not None
        return _capi.activate_backward(rotation_raw.contiguous(), scales, opac, g_scales, g_rot, g_opac,
                                       g_shs.contiguous())


class _StashingActivations(torch.autograd.Function):
    """FusedActivations for the fused optimiser tail (FusedAdam.step_model): forward hands out the activated
    values the last step already computed (no launch) or computes them; backward does NOT run the chain rule -- it
    parks the gradients w.r.t. the activated tensors on the model, and FusedAdam.step_model applies chain rule +
    Adam + next activations in one kernel (csrc/optimizer.hip, k_model_step)."""

    @staticmethod
    def forward(ctx, model, scaling_raw, rotation_raw, opacity_raw, features_dc, features_rest):
        ctx.model = model
        cached = model._next_act
        model._next_act = None
        if cached is not None:
            return cached
        return _capi.activate(scaling_raw.contiguous(), rotation_raw.contiguous(), opacity_raw.contiguous(),
                              features_dc.contiguous(), features_rest.contiguous())

    @staticmethod
    def backward(ctx, g_scales, g_rot, g_opac, g_shs):
        m = ctx.model
        new = [g_scales, g_rot, g_opac, g_shs]
        shapes = [(m._scaling.shape), (m._rotation.shape), (m._opacity.shape),
                  (m._xyz.shape[0], 1 + m._features_rest.shape[1], 3)]
        new = [torch.zeros(sh, device=m._xyz.device) if g is None else g.contiguous() for g, sh in zip(new, shapes)]
        if m._act_grads is None:
            m._act_grads = new
        else:  # several backward passes before one step (views rendered in separate graphs): gradients add up
            m._act_grads = [a + b for a, b in zip(m._act_grads, new)]
        return None, None, None, None, None, None


class GaussianParameters(torch.nn.Module):
    """The leaf tensors of GaussianModel (include/gs/gs/gaussian.cuh:107-119) and its getters."""

    def __init__(self, xyz, features_dc, features_rest, scaling, rotation, opacity):
        super().__init__()
        P = torch.nn.Parameter
        self._xyz, self._features_dc, self._features_rest = P(xyz), P(features_dc), P(features_rest)
        self._scaling, self._rotation, self._opacity = P(scaling), P(rotation), P(opacity)
        self._init_fused_tail()

    def _init_fused_tail(self):
        self.fused_tail = False   # True: activated() parks gradients for FusedAdam.step_model (see there)
        self._next_act = None     # activated values of the current parameters, left by the last step_model
        self._act_grads = None    # gradients w.r.t. (scales, rotations, opacities, shs) parked by backward

    def activated(self):
        """(xyz, opacity [P,1], scales, rotations, shs) through one fused node."""
        if self.fused_tail:
            scales, rot, opac, shs = _StashingActivations.apply(self, self._scaling, self._rotation, self._opacity,
                                                                self._features_dc, self._features_rest)
        else:
            scales, rot, opac, shs = FusedActivations.apply(self._scaling, self._rotation, self._opacity,
                                                            self._features_dc, self._features_rest)
        return self._xyz, opac, scales, rot, shs

    # reference getter names (each call runs the fused node; use activated() to get all at once)
    def Get_xyz(self):
        return self._xyz

    def Get_max_sh_degree(self):
        m = 1 + int(self._features_rest.shape[1])  # coefficients per channel = (degree + 1)^2
        return int(round(m ** 0.5)) - 1

    def Get_opacity(self):
        return self.activated()[1]

    def Get_scaling(self):
        return self.activated()[2]

    def Get_rotation(self):
        return self.activated()[3]

    def Get_features(self):
        return self.activated()[4]

    def param_groups(self, position_lr=0.0005, feature_lr=0.001, opacity_lr=0.025, scaling_lr=0.0025,
                     rotation_lr=0.0025, spatial_lr_scale=1.0):
        """Groups and learning rates of GaussianModel::Training_setup (src/gs/gaussian.cu:396-428) with the
        defaults of config/basic_common.yaml:54-62."""
        return [
            {"params": [self._xyz], "lr": position_lr * spatial_lr_scale},
            {"params": [self._features_dc], "lr": feature_lr},
            {"params": [self._features_rest], "lr": feature_lr / 20.0},
            {"params": [self._scaling], "lr": scaling_lr * spatial_lr_scale},
            {"params": [self._rotation], "lr": rotation_lr},
            {"params": [self._opacity], "lr": opacity_lr},
        ]


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (no weight decay / amsgrad), all groups in ONE kernel launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-15):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._step = 0

    @torch.no_grad()
    def step(self, zero_grads=True):
        ps, gs, ms, vs, lrs = [], [], [], [], []
        betas = eps = None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                assert betas in (None, group["betas"]) and eps in (None, group["eps"]), \
                    "FusedAdam: one (betas, eps) for all groups, as the reference configures it"
                betas, eps = group["betas"], group["eps"]
                ps.append(p); gs.append(p.grad); ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"])
                lrs.append(group["lr"])
        self._step += 1
        for i in range(0, len(ps), 8):
            _capi.adam_step(ps[i:i + 8], gs[i:i + 8], ms[i:i + 8], vs[i:i + 8], lrs[i:i + 8], betas[0], betas[1],
                            eps, self._step, zero_grads)

    @torch.no_grad()
    def step_model(self, model):
        """The optimiser tail of one iteration in ONE launch (k_model_step): chain rule of the activations, Adam on
        the six groups of `model` (which must be this optimiser's six groups, `model.fused_tail = True`), and the
        activated values of the updated parameters, which the next `model.activated()` hands out without a launch.
        Equivalent to FusedActivations' backward + step(); the raw-space gradients are never materialised."""
        assert model.fused_tail and model._act_grads is not None and model._xyz.grad is not None, \
            "step_model needs a backward through model.activated() with model.fused_tail = True"
        ps = [model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity]
        lrs, ms, vs = [], [], []
        betas, eps = self.defaults["betas"], self.defaults["eps"]
        for p in ps:
            if p.numel() == 0:  # e.g. features_rest at SH degree 0: nothing to step, its group may be absent
                lrs.append(0.0); ms.append(p.detach()); vs.append(p.detach())
                continue
            grp = next(g for g in self.param_groups if any(q is p for q in g["params"]))
            st = self.state[p]
            if not st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            lrs.append(grp["lr"]); ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"])
            betas, eps = grp["betas"], grp["eps"]
        self._step += 1
        g_scales, g_rot, g_opac, g_shs = model._act_grads
        model._next_act = _capi.model_step(ps, ms, vs, model._xyz.grad.contiguous(), g_scales, g_rot, g_opac, g_shs, lrs,
                                           betas[0], betas[1], eps, self._step)
        model._act_grads = None
        model._xyz.grad = None


class VoxelIndex:
    """voxel key -> (first_row, count): the rows of the Gaussians a voxel contributed to the model.

    The reference keeps one std::vector<int> of row numbers per key (gs_hash_indexes_, filled by addNewPointcloud,
    src/gs/gaussian.cu:257-263), but those vectors are always an iota from the running model size
    (src/liw/lioOptimization.cpp:1268-1279), so a range says the same.  A duplicate key is an error, as there
    (:258-262, where it ends the program); a voxel whose sample was empty registers a key without rows (:1268-1273).
    """

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self._ranges = {}

    def __len__(self):
        return len(self._ranges)

    def __contains__(self, key):
        return int(key) in self._ranges

    def get(self, key):
        """(first_row, count) of a key, or None."""
        return self._ranges.get(int(key))

    def add(self, keys, counts, first_row):
        """Registers len(keys) voxels whose Gaussians lie one after another from `first_row`; returns the row after
        the last.  Raises (and registers nothing) on a key that is already known or given twice."""
        keys = [int(k) for k in keys]
        counts = [int(c) for c in counts]
        if len(keys) != len(counts):
            raise ValueError("VoxelIndex.add: %d keys, %d counts" % (len(keys), len(counts)))
        if any(c < 0 for c in counts):
            raise ValueError("VoxelIndex.add: negative count")
        seen = set()
        for k in keys:
            if k in self._ranges or k in seen:
                raise KeyError("VoxelIndex.add: voxel key %d duplicated" % k)
            seen.add(k)
        row = int(first_row)
        for k, c in zip(keys, counts):
            self._ranges[k] = (row, c)
            row += c
        return row

    def remap(self, row_map):
        """Follows a stable compaction of the model's rows (GrowableGaussians.prune): row_map [P+1] (host integers) is
        the exclusive prefix sum of "kept", so a key's (first, count) becomes
        (row_map[first], row_map[first + count] - row_map[first]) -- a range stays a range.  A voxel that loses all its
        rows stays registered with count 0 (adding its key again is still the duplicate-key error).  Host only, one
        vectorised pass over the keys.  Raises (and changes nothing) when a range ends beyond the P rows of row_map."""
        rm = row_map.cpu().numpy() if isinstance(row_map, torch.Tensor) else np.asarray(row_map)
        rm = rm.astype(np.int64).reshape(-1)
        if rm.size == 0:
            raise ValueError("VoxelIndex.remap: row_map has P + 1 entries")
        if not self._ranges:
            return
        keys = list(self._ranges)
        rng = np.array([self._ranges[k] for k in keys], dtype=np.int64).reshape(-1, 2)
        first, end = rng[:, 0], rng[:, 0] + rng[:, 1]
        if int(first.min()) < 0 or int(end.max()) > rm.size - 1:
            raise ValueError("VoxelIndex.remap: a voxel's rows end at %d, row_map covers %d rows"
                             % (int(end.max()), rm.size - 1))
        new_first = rm[first]
        new_count = rm[end] - new_first
        self._ranges = dict(zip(keys, zip(new_first.tolist(), new_count.tolist())))

    def select(self, losses, max_points=500, generator=None):
        """Steps 1-2 of GaussianModel::calcSimiLoss (src/gs/gaussian.cu:201-228) on the host.

        losses: {voxel key: [k,3] f32 CPU tensor}, GsForLosses::_losses as processAndMergeLosses leaves it
        (src/liw/lioOptimization.cpp:459-476).  Every key this index knows contributes its rows and its points (in
        ascending key order, so that the result does not depend on the order of the map), the others neither.
        `max_points` or more points are cut to exactly `max_points` by torch.randperm on the CPU (:226-228, MAX_SIMI).
        Returns (points [m,3] f32, sel [n] int32 = the ascending unique rows, what loss_mask.nonzero() yields) on
        `self.device` through non-blocking copies, or None where the reference returns false (no point left) and
        where it has no Gaussian to compare with (every matched voxel empty)."""
        ranges = self._ranges
        hit = sorted(k for k in losses if k in ranges)
        if not hit:
            return None
        pts = [losses[k] for k in hit]
        if not all(type(t) is torch.Tensor and t.dtype == torch.float32 and t.dim() == 2 for t in pts):
            pts = [torch.as_tensor(t, dtype=torch.float32).reshape(-1, 3) for t in pts]  # (arrays, lists, [3] rows)
        points = torch.cat(pts, 0) if len(pts) > 1 else pts[0]
        m = int(points.size(0))
        rng = np.array([ranges[k] for k in hit], dtype=np.int64).reshape(-1, 2)
        rng = rng[rng[:, 1] > 0]
        if m == 0 or rng.shape[0] == 0:
            return None
        rng = rng[np.argsort(rng[:, 0], kind="stable")]
        first, count = rng[:, 0], rng[:, 1]
        # rows of all ranges, one after another: each range's own iota = global iota - (rows before it) + its first
        before = np.cumsum(count) - count
        rows = np.arange(int(count.sum()), dtype=np.int64) + np.repeat(first - before, count)
        if np.any(first[1:] < first[:-1] + count[:-1]):  # overlapping ranges (not what add() lays out, but legal)
            rows = np.unique(rows)
        if m >= max_points:
            keep = torch.randperm(m, generator=generator)[:max_points]
            points = points.index_select(0, keep)
        sel = torch.from_numpy(rows.astype(np.int32))
        points = points.contiguous()
        if self.device.type == "cuda":  # pinned staging: the copies are queued, the host does not wait for them
            sel, points = sel.pin_memory(), points.pin_memory()
        return points.to(self.device, non_blocking=True), sel.to(self.device, non_blocking=True)


class GrowableGaussians(GaussianParameters):
    """The six leaves and their Adam moments as CAPACITY buffers; the leaves are views of the first P rows.

    The reference grows the map every few frames by building the new rows with Torch ops and then
    `torch::cat`-ing ALL six parameter tensors and all twelve optimiser-state tensors (whole-model copies,
    src/gs/gaussian.cu:451-472, 524-540).  Here `add_new_pointcloud` initialises rows [P, P + n) in place with
    one kernel (csrc/growth.hip) and re-binds the leaves: O(n) bytes move; the moments of the new rows are the
    zeros the buffers were created with (= the reference's `zeros_like(extension_tensor)`), the step count is
    shared (= the reference keeps the old AdamParamState's step).  When the capacity is exhausted the buffers
    double (one amortised copy).
    """

    _NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")

    def __init__(self, capacity, M, device):
        torch.nn.Module.__init__(self)
        self._init_fused_tail()
        self.M, self.P, self.capacity, self.device = int(M), 0, 0, torch.device(device)
        self._buf, self._m, self._v = {}, {}, {}
        self._optimizer = None
        self._stats = None  # [capacity, 3] {grad_sum, views, max_radius}: enable_density_stats()
        self._cstats = None  # [capacity, 3] {weight_sum_total, views, weight_max}: enable_contribution_stats()
        self._visibility = []  # covis.KeyframeVisibility records that follow a prune: attach_visibility()
        self.voxel_index = VoxelIndex(self.device)  # gs_hash_indexes_
        self._reserve(max(1, int(capacity)))
        self._bind()

    def _shapes(self):
        return {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (self.M - 1, 3), "_scaling": (3,),
                "_rotation": (4,), "_opacity": (1,)}

    def _reserve(self, capacity):
        for name, tail in self._shapes().items():
            for store in (self._buf, self._m, self._v):
                new = torch.zeros((capacity,) + tail, dtype=torch.float32, device=self.device)
                if name in store and self.P:
                    new[:self.P].copy_(store[name][:self.P])
                store[name] = new
        if self._stats is not None:
            new = torch.zeros((capacity, 3), dtype=torch.float32, device=self.device)
            new[:self.P].copy_(self._stats[:self.P])
            self._stats = new
        if self._cstats is not None:
            new = torch.zeros((capacity, 3), dtype=torch.float32, device=self.device)
            new[:self.P].copy_(self._cstats[:self.P])
            self._cstats = new
        self.capacity = capacity

    def _bind(self):
        """Leaves = views of the first P rows (new Parameter objects, same storage); optimiser state follows."""
        for name in self._NAMES:
            setattr(self, name, torch.nn.Parameter(self._buf[name][:self.P]))
        self._next_act = None  # the cached activations describe the old row count
        self._act_grads = None  # ... and so would gradients parked by a backward that ran before the growth
        if self._optimizer is not None:
            self._optimizer.rebind(self)

    def moments(self, name):
        return self._m[name][:self.P], self._v[name][:self.P]

    def attach(self, optimizer):
        self._optimizer = optimizer

    def attach_visibility(self, vis):
        """Makes `prune` renumber the keyframe visibility records `vis` (covis.KeyframeVisibility) with the rows: one
        launch on the device row map, only when rows were dropped, before prune returns.  Growth needs nothing: new rows
        keep the old numbers and older keyframes read 0 for them.  Without an attachment prune launches what it always
        launched."""
        if not any(v is vis for v in self._visibility):
            self._visibility.append(vis)

    @torch.no_grad()
    def add_new_pointcloud(self, xyz, covs, rgbs, scale_factor=1.0, voxel_keys=None, voxel_counts=None):
        """GaussianModel::addNewPointcloud (src/gs/gaussian.cu:241-313): xyz [n,3], covs [n,3,3], rgbs [n,3] (0..255),
        device f32.  Returns the row range of the new Gaussians.
        voxel_keys / voxel_counts (optional, host sequences): the voxels the points came from, in the order of the
        rows, and how many rows each contributed (pcd.hash_posi_s / pcd.indexes, :257-263); they are registered in
        `self.voxel_index` at [P_old, ...).  A duplicate key or counts that do not sum to n raise before anything
        changes."""
        n = int(xyz.size(0))
        if (voxel_keys is None) != (voxel_counts is None):
            raise ValueError("add_new_pointcloud: voxel_keys and voxel_counts go together")
        if voxel_keys is not None:
            if sum(int(c) for c in voxel_counts) != n:
                raise ValueError("add_new_pointcloud: voxel_counts sum to %d, %d rows given"
                                 % (sum(int(c) for c in voxel_counts), n))
            self.voxel_index.add(voxel_keys, voxel_counts, self.P)
        if n == 0:
            return self.P, self.P
        if self.P + n > self.capacity:
            self._reserve(max(2 * self.capacity, self.P + n))
        lo, hi = self.P, self.P + n
        b = self._buf
        _capi.init_gaussians(xyz.contiguous(), covs.contiguous(), rgbs.contiguous(), scale_factor, b["_xyz"][lo:hi],
                             b["_features_dc"][lo:hi], b["_features_rest"][lo:hi], b["_scaling"][lo:hi],
                             b["_rotation"][lo:hi], b["_opacity"][lo:hi])
        self.P = hi
        self._bind()
        return lo, hi

    @torch.no_grad()
    def add_unexplained(self, points_world, camera, depth, acc, image, scale_factor=1.0, **admit_arguments):
        """Seeds Gaussians only where the map lacks them: `admit_sweep` (seed.py) of a sweep against the render
        (depth, acc: the rasterizer's second and third outputs, or None for both while there is no model) and the
        image ([3,H,W], 0..1) of `camera` (a render_utils.Camera: its pose through `world_to_camera`, its intrinsics
        through `raster_K`), then `add_new_pointcloud` of the admitted points.  admit_arguments: depth_tol and
        occlusion_tol (required) and admit_sweep's other keywords.  The appended rows belong to no voxel, as
        densify's; group by the returned indices to register voxels.  One host wait (the admitted count).
        Returns (lo, hi, counts): the row range of the new Gaussians and admit_sweep's six counts."""
        from .loss import raster_K, world_to_camera
        from .seed import admit_sweep
        W, H = camera.Get_image_width(), camera.Get_image_height()
        a = admit_sweep(points_world, world_to_camera(camera), raster_K(W, H, camera.Get_FoVx(), camera.Get_FoVy()), H, W,
                        depth=depth, acc=acc, image=image, **admit_arguments)
        lo, hi = self.add_new_pointcloud(a.xyz, a.covs, a.rgbs, scale_factor)
        return lo, hi, a.counts

    @torch.no_grad()
    def add_voxel_seeds(self, seeds, oriented=True, scale_factor=1.0):
        """Appends the Gaussians of voxelmap.SweepVoxelMap.sweep (`seeds`, a VoxelSeeds from a sweep WITH colours), one
        per matured voxel, each registered in `self.voxel_index` under its voxel key with count 1 -- so that
        calc_simi_loss selects them.  `add_new_pointcloud` initialises the rows (from the covariances' diagonals, as it
        always does, with `scale_factor`); with `oriented` the scaling and the rotation are then overwritten by the
        seeds' own, which hold the SWEEP's scale_factor: flat surfels along the voxel's axes instead of axis-aligned
        boxes.  oriented=False is exactly add_new_pointcloud.  Returns the row range."""
        if seeds.rgbs is None:
            raise ValueError("add_voxel_seeds: the sweep had no colours")
        v = int(seeds.xyz.size(0))
        lo, hi = self.add_new_pointcloud(seeds.xyz, seeds.covs, seeds.rgbs, scale_factor,
                                         voxel_keys=seeds.keys.tolist(), voxel_counts=[1] * v)
        if oriented and v:
            self._buf["_scaling"][lo:hi].copy_(seeds.scaling_raw)
            self._buf["_rotation"][lo:hi].copy_(seeds.rotation)
        return lo, hi

    @torch.no_grad()
    def prune(self, min_opacity=1.0 / 255.0, max_scale=0.3, drop_nonfinite=True, drop=None):
        """Removes the rows that are dead to the rasterizer for good -- the shrinking counterpart of add_new_pointcloud,
        GaussianModel::prune_optimizer (src/gs/gaussian.cu:430-449) for all six groups at once.  A row leaves when
          * sigmoid(_opacity) < min_opacity: below 1/255 its alpha never reaches the blend's 1/255 test, forward or
            backward, so it contributes to no pixel and gets no photometric gradient;
          * any exp(_scaling) > max_scale: k_preprocess' scale cull (at scale_modifier 1) drops it outright -- no tiles,
            no gradient, nothing that would bring the scale back;
          * drop_nonfinite and any of xyz / scaling / rotation / opacity is NaN or +-Inf;
          * drop (optional [P] bool or uint8 device tensor) marks it.
        Values ON a threshold stay (the rasterizer culls on >).  The survivors keep their order (a stable compaction),
        so `voxel_index` ranges stay ranges and depth ties fall as before; with the defaults no pixel and no survivor's
        gradient changes.  The Adam moments move with their rows, rows [P', capacity) of both moments are zero
        afterwards (add_new_pointcloud relies on that), the step count and the capacity are kept.
        Cost: four launches, ONE host wait per prune (the copy of the row map, which carries P'), and a transient
        second set of capacity buffers (the compaction is out of place); the old set is released on return.
        When nothing is dropped nothing is moved or re-bound: leaf objects and cached activations survive.  Otherwise
        the leaves are new Parameter objects (as after a growth), cached activations and parked gradients are
        dropped, and a `sel` obtained from `voxel_index.select` BEFORE the prune is stale: select again.
        Returns {"P_before", "P_after", "n_opacity", "n_scale", "n_nonfinite", "n_mask" (a row with several reasons
        counts under each), "row_map": [P+1] int32 on the host, row_map[i] = new row of old row i, row_map[P] = P',
        "reasons": [P] uint8 on the device, 0 = kept}."""
        P, b = self.P, self._buf
        if drop is not None:
            drop = drop.to(self.device).reshape(-1).contiguous()
            if drop.numel() != P:
                raise ValueError("prune: drop has %d entries, the model %d rows" % (drop.numel(), P))
        reasons, row_map, _, both = _capi.prune_mark(b["_xyz"][:P], b["_scaling"][:P], b["_rotation"][:P],
                                                     b["_opacity"][:P], min_opacity, max_scale, drop_nonfinite, drop,
                                                     packed=True)
        host = both.cpu()  # the one host wait
        row_map_host, counts = host[:P + 1], [int(c) for c in host[P + 1:]]
        P_new = counts[0]
        out = dict(P_before=P, P_after=P_new, n_opacity=counts[1], n_scale=counts[2], n_nonfinite=counts[3],
                   n_mask=counts[4], row_map=row_map_host, reasons=reasons)
        if P_new == P:
            return out
        src, dst, fresh = [], [], ({}, {}, {})
        for name, tail in self._shapes().items():
            for store, new in zip((self._buf, self._m, self._v), fresh):
                new[name] = torch.zeros((self.capacity,) + tail, dtype=torch.float32, device=self.device)
                src.append(store[name][:P])
                dst.append(new[name])
        _capi.prune_compact(src, dst, reasons, row_map)
        if self._stats is not None:  # the statistics follow their rows (a second launch: the first carries 18 tensors)
            stats = torch.zeros((self.capacity, 3), dtype=torch.float32, device=self.device)
            _capi.prune_compact([self._stats[:P]], [stats], reasons, row_map)
            self._stats = stats
        if self._cstats is not None:  # ... and so do the contribution statistics
            cstats = torch.zeros((self.capacity, 3), dtype=torch.float32, device=self.device)
            _capi.prune_compact([self._cstats[:P]], [cstats], reasons, row_map)
            self._cstats = cstats
        self._buf, self._m, self._v = fresh
        self.P = P_new
        self._bind()
        self.voxel_index.remap(row_map_host)
        for vis in self._visibility:
            vis.remap(reasons, row_map, rows_after=P_new)
        return out

    @torch.no_grad()
    def enable_density_stats(self):
        """Creates the zero [capacity, 3] statistics buffer {grad_sum, views, max_radius} that accumulate_density
        fills and densify reads.  A model that never calls this runs none of the density-control code."""
        if self._stats is None:
            self._stats = torch.zeros((self.capacity, 3), dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def enable_contribution_stats(self):
        """Creates the zero [capacity, 3] statistics buffer {weight_sum_total, views, weight_max} that
        contribution(..., stats=model.contribution_stats()) folds a view into (contribution.py).  `prune` compacts it
        with its rows; rows appended by `densify` and `add_new_pointcloud` start at zero.  A model that never calls this
        runs none of the contribution code."""
        if self._cstats is None:
            self._cstats = torch.zeros((self.capacity, 3), dtype=torch.float32, device=self.device)

    def contribution_stats(self):
        """The contribution statistics of the P rows, a [P, 3] view (None before enable_contribution_stats)."""
        return None if self._cstats is None else self._cstats[:self.P]

    @torch.no_grad()
    def reset_contribution_stats(self):
        """Zeroes the contribution statistics (the start of a new sweep over the keyframes)."""
        if self._cstats is not None:
            self._cstats.zero_()

    def density_stats(self):
        """The statistics of the P rows, a [P, 3] view (None before enable_density_stats)."""
        return None if self._stats is None else self._stats[:self.P]

    @torch.no_grad()
    def accumulate_density(self, radii, means2D_grad):
        """One view's statistics, one launch, after that view's backward: radii [P] int32 as the forward returned them,
        means2D_grad [P,3] = the .grad of the means2D leaf (render_utils.render_full), unscaled.  Rows the view did
        not see (radii <= 0) and rows with a non-finite gradient norm are not touched."""
        if self._stats is None:
            raise RuntimeError("accumulate_density: call enable_density_stats() first")
        if int(radii.numel()) != self.P or tuple(means2D_grad.shape) != (self.P, 3):
            raise ValueError("accumulate_density: the model has %d rows" % self.P)
        if self.P:
            _capi.density_accumulate(radii.contiguous(), means2D_grad.contiguous(), self._stats[:self.P])

    @torch.no_grad()
    def densify(self, grad_threshold, size_threshold, max_new=None, seed=0):
        """Adaptive density control, the growing counterpart of prune (upstream's densify_and_clone and
        densify_and_split with N = 2; include/gsraster.h has the full contract).  A row whose mean view-space gradient
        norm grad_sum / views is >= grad_threshold (in the units of gsr_backward's dL_dmean2D, unscaled) is a candidate:
        with max exp(_scaling) <= size_threshold it is CLONED -- the copy is appended, the parent keeps its Adam
        moments, the copy starts with zeros --, above it it is SPLIT -- the parent becomes the first child in place, the
        second child is appended, both 1.6 times smaller, displaced by normal samples of the parent's own shape, with
        zero moments.  Every candidate appends exactly one row; max_new caps the rows added (the first max_new
        candidates in row order win); the samples depend on (seed, row, child) only.
        Existing rows keep their numbers, so a `sel` taken from `voxel_index.select` BEFORE densify remains valid and
        `voxel_index` is unchanged.  The appended rows belong to NO voxel of `voxel_index`: the similarity loss never
        selects them, and a later prune moves them like any other row.
        Cost: four launches and ONE host wait (the copy of the offsets, which carries the count); when the capacity is
        exceeded the buffers grow first, as in add_new_pointcloud.  The statistics are zero afterwards.  When nothing is
        added nothing is re-bound: leaf objects and cached activations survive; otherwise the leaves are new Parameter
        objects and cached activations and parked gradients are dropped.
        Returns {"P_before", "P_after", "n_new", "n_clone", "n_split", "kinds": [P] uint8 on the device (0 none,
        1 clone, 2 split), "offsets": [P+1] int32 on the host, row i's new row is P_before + offsets[i]}."""
        if self._stats is None:
            raise RuntimeError("densify: call enable_density_stats() first")
        P, b = self.P, self._buf
        kinds, offsets, _, both = _capi.densify_mark(self._stats[:P], b["_scaling"][:P], grad_threshold, size_threshold,
                                                     max_new, packed=True)
        host = both.cpu()  # the one host wait
        n_new, n_clone, n_split = (int(c) for c in host[P + 1:])
        out = dict(P_before=P, P_after=P + n_new, n_new=n_new, n_clone=n_clone, n_split=n_split, kinds=kinds,
                   offsets=host[:P + 1])
        if n_new:
            if P + n_new > self.capacity:
                self._reserve(max(2 * self.capacity, P + n_new))
            b = self._buf
            _capi.densify_apply(P, n_new, kinds, offsets, seed, [b[n] for n in self._NAMES],
                                [self._m[n] for n in self._NAMES], [self._v[n] for n in self._NAMES], self._stats)
            self.P = P + n_new
            self._bind()
        self._stats[:self.P].zero_()
        return out

    def calc_simi_loss(self, losses, lambda_=0.2, scaling=None, max_points=500, generator=None):
        """GaussianModel::calcSimiLoss (src/gs/gaussian.cu:201-239): the similarity loss of the LiDAR points in
        `losses` ({voxel key: [k,3] CPU f32}) against the Gaussians of their voxels, or None where the reference
        returns false.  scaling: the activated scales of this iteration's `activated()` call, so that the term shares
        the rasterizer's node; None runs the getter, as the reference does."""
        from .loss import similarity_loss
        picked = self.voxel_index.select(losses, max_points=max_points, generator=generator)
        if picked is None:
            return None
        points, sel = picked
        if scaling is None:
            scaling = self.Get_scaling()
        return similarity_loss(points, sel, self._xyz, scaling, lambda_)

    def calc_plane_loss(self, losses, lambda_, scaling=None, rotation=None, huber=0.0, max_dist=float("inf"),
                        lambda_flat=0.0, max_points=500, generator=None):
        """The point-to-plane term (loss.surfel_plane_loss) on calc_simi_loss's selection: the LiDAR points in `losses`
        against the thinnest axis of their nearest Gaussian among those of their voxels, or None where calc_simi_loss
        returns None.  scaling, rotation: the activated values of this iteration's `activated()` call, so that the
        term shares the rasterizer's node on both activation paths; None runs the getter."""
        from .loss import surfel_plane_loss
        picked = self.voxel_index.select(losses, max_points=max_points, generator=generator)
        if picked is None:
            return None
        points, sel = picked
        if scaling is None or rotation is None:
            _, _, act_scaling, act_rotation, _ = self.activated()
            scaling = act_scaling if scaling is None else scaling
            rotation = act_rotation if rotation is None else rotation
        return surfel_plane_loss(points, sel, self._xyz, scaling, rotation, lambda_, huber, max_dist, lambda_flat)


@torch.no_grad()
def prune_rows(tensors, reasons, row_map, P_new):
    """For callers who hold plain tensors: the rows of each [P, ...] f32 device tensor with reasons[i] == 0, in order,
    as new [P_new, ...] tensors -- t[reasons == 0] for all of them, eighteen per launch (csrc/prune.hip).
    reasons / row_map: what _capi.prune_mark returned; P_new = int(row_map[P]), which the caller has fetched."""
    tensors = [t.contiguous() for t in tensors]
    P_new = int(P_new)
    outs = [torch.empty((P_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in tensors]
    for i in range(0, len(tensors), 18):
        _capi.prune_compact(tensors[i:i + 18], outs[i:i + 18], reasons, row_map)
    return outs


class GrowableAdam(FusedAdam):
    """FusedAdam whose moments live in the model's capacity buffers, so growing the model needs no optimiser-state
    concatenation (cat_tensors_to_optimizer, src/gs/gaussian.cu:451-472)."""

    def __init__(self, model, eps=1e-15, **lrs):
        self._lrs = lrs
        super().__init__(model.param_groups(**lrs), eps=eps)
        model.attach(self)
        self.rebind(model)

    def rebind(self, model):
        groups = model.param_groups(**self._lrs)
        for g_old, g_new in zip(self.param_groups, groups):
            g_old["params"] = g_new["params"]
        self.state.clear()
        for name in model._NAMES:
            p = getattr(model, name)
            m, v = model.moments(name)
            self.state[p] = {"exp_avg": m, "exp_avg_sq": v}
