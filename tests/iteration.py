"""One whole optimiser iteration, every loss term at once: the session, the by-hand route and the bars (test
infrastructure; tests/test_iteration_cases.py runs the host-only half, tests/test_gpu_iteration.py the rest).

The scene.  600 Gaussians of S.make_scene(600, 70, 50, 21, sh_degree=1) with three times the scales, seen at 70 x 50
(5 x 4 tiles, partial on both edges) by three cameras at 60 degrees: the identity, rotation(2, -1.5, 3) at
(0.06, -0.02, 0.03) and rotation(-1, 1, -2.5) at (-0.05, 0.03, -0.02).  A LiDAR sweep (the plane of
test_gpu_lidar._loop, in camera 0's frame = the world), delta pairs (0 -> 1) and (1 -> 2), 257 similarity points
around rows [100, 260), per-view targets with their own gain and bias, a [3,2] exposure leaf for views 0 and 1 and a
shared log-gain [2] leaf for view 2, one zero pose leaf per camera.  Weights: none is 1.0 or a power of two, so a
backward that forgets its upstream factor cannot hide.

Route A, the product: `Session.run()` -- render_full four times per iteration (camera 0 twice; the second render
carries a plain photometric term), the five loss functions, total = sum_k float32(w_k) t_k, ONE backward,
accumulate_density per render, FusedAdam.step_model, a plain Adam step on exposures and pose leaves, Camera.retract.
Three iterations; densify and prune between the second and the third.  Every tensor that reaches or leaves the host
code is cloned into the iteration's record.

Route B, by hand: `replay(static, rec)` -- from A's record of one iteration, with no autograd: _capi.activate,
_capi.rasterize_forward, each loss's _capi entry for upstream 1, the scaling and masking written out, the sums over
consumers in FLOAT64, _capi.rasterize_backward fed with A's retained image gradients, _capi.pose_gradient,
_capi.similarity_loss and _capi.model_step on clones.  Every stage of B is pinned to float64 by its own test file, so
A = B pins the composition: the host code between the kernels.

Bars (`compare`).  Either equality of every bit, or the join bar

    J(s_1 .. s_n) = (n - 1) * 2^-23 * sum_i |s_i|

for a quantity autograd forms by n - 1 float32 additions in an order of its own choosing: each addition rounds once,
by at most 2^-24 of a partial sum that is at most sum_i |s_i| -- counted at a whole 2^-23 as delta_ref and lidar_ref
count.  The shared log-gain exposure adds two roundings (expf and its product) on the same magnitude.

Float64 anchors, evaluated at A's own float32 values so that no stage inherits another's rounding: `image_anchor` (the
composed image-level loss from exposure_ref, loss_ref, lidar_ref and delta_ref, all three iterations), `leaf_anchor`
(depth_ref.render64 per render, summed, plus simi_ref and pose_ref; iteration 1) and, in the test file, the step
against optim_ref.  The shares of the scene are stated and asserted in whole per cent (tests/test_iteration_cases.py).
"""
import functools
import math

import numpy as np
import torch

import poses
from gs_livm_amd import synthetic as S

W, H = 70, 50
P0 = 600
EPS32 = 2.0 ** -23
FOVX = math.radians(60.0)
FOVY = 2.0 * math.atan(math.tan(FOVX / 2.0) * H / W)
POSES = ((dict(), (0.0, 0.0, 0.0)),
         (dict(roll=2.0, pitch=-1.5, yaw=3.0), (0.06, -0.02, 0.03)),
         (dict(roll=-1.0, pitch=1.0, yaw=-2.5), (-0.05, 0.03, -0.02)))
RENDERS = (0, 1, 2, 0)                       # the camera of each render of an iteration
PAIRS = ((0, 1), (1, 2))                     # delta-depth (source view, reference view)
WEIGHTS = dict(photo=0.8, lidar=0.35, delta=1.3, simi=0.6)
LAMBDAS = dict(photo=0.2, lidar=0.7, delta=0.2, simi=0.2)
ACC_MIN = 0.5
GAINS, BIASES = (1.2, 1.0, 0.85), (0.03, 0.0, -0.02)
SEL_ROWS = (100, 260)                        # 10 voxels of 16 rows
VOXEL_KEYS = tuple(7000 + 13 * i for i in range(10))
REST_KEY = 99991                             # the voxel of rows [260, 600): never in `losses`, never selected
M_POINTS = 257
MARGIN = 1e-3
ITERATIONS = 3
# adaptive density control between iterations 2 and 3 (tests/test_iteration_cases.py holds both to "moves the count")
DENSIFY = dict(grad_threshold=0.03, size_threshold=0.1)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
_ROWS = ((0.8, -0.05), (1.0, 0.0), (1.25, 0.1))   # exposure_ref.ROWS: every channel its own row, off the identity
EXPOSURES = (_ROWS, _ROWS[1:] + _ROWS[:1], (0.1, -0.02))   # views 0 and 1: [3,2]; view 2: shared (log gain, bias)


# ---- host-only data (numpy / CPU torch; nothing here touches the device) ---------------------------------------------
@functools.lru_cache(maxsize=1)
def scene():
    sc = S.make_scene(P0, W, H, 21, sh_degree=1)
    sc["scales"] = (sc["scales"] * 3.0).astype(np.float32)
    return sc


@functools.lru_cache(maxsize=1)
def cameras():
    return tuple(poses.camera(W, H, poses.rotation(**rpy), np.array(T)) for rpy, T in POSES)


def view_scene(v, sc=None):
    out = dict(scene() if sc is None else sc)
    out.update(cameras()[v])
    return out


@functools.lru_cache(maxsize=1)
def oracle_frames():
    from oracle import oracle as O
    return tuple(O.forward(view_scene(v), keep_handle=False) for v in range(3))


@functools.lru_cache(maxsize=1)
def keep_masks():
    """[3][1,H,W] float32 0/1: the oracle's `fragile == 0` on the starting state, constant over the session."""
    return tuple(torch.from_numpy((fr.fragile == 0).astype(np.float32))[None] for fr in oracle_frames())


@functools.lru_cache(maxsize=1)
def targets():
    """Per view: the oracle's image of the scene with SH dc * 0.9 and means shifted, times the view's gain, plus its
    bias, clipped to [0, 1]."""
    from oracle import oracle as O
    sc = dict(scene())
    shs = sc["shs"].copy()
    shs[:, 0, :] *= np.float32(0.9)
    sc["shs"] = shs
    sc["means3D"] = (sc["means3D"] + np.array([0.01, -0.01, 0.02], np.float32)).astype(np.float32)
    out = []
    for v in range(3):
        img = O.forward(view_scene(v, sc), keep_handle=False).out_color
        out.append(torch.from_numpy(np.clip(img * np.float32(GAINS[v]) + np.float32(BIASES[v]), 0.0, 1.0)
                                    .astype(np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def sweep():
    """The plane of test_gpu_lidar._loop (seed 4, two points per pixel, z = 4.5 +- 0.3) in camera 0's frame."""
    rng = np.random.default_rng(4)
    n = 2 * W * H
    zc = 4.5 + 0.3 * rng.uniform(-1, 1, n)
    return np.stack([rng.uniform(-0.7, 0.7, n) * zc, rng.uniform(-0.5, 0.5, n) * zc, zc], 1).astype(np.float32)


def raster_K():
    fx, fy = W / (2.0 * math.tan(FOVX * 0.5)), H / (2.0 * math.tan(FOVY * 0.5))
    return np.array([[fx, 0.0, (W - 1) * 0.5], [0.0, fy, (H - 1) * 0.5], [0.0, 0.0, 1.0]], np.float64)


def world_to_camera(v):
    """[3,4] float32 [R | t] of view v's starting pose, from the transposed view matrix."""
    return np.ascontiguousarray(cameras()[v]["viewmatrix"].T[:3]).astype(np.float32)


@functools.lru_cache(maxsize=1)
def quat_factors():
    return np.random.default_rng(33).uniform(0.5, 2.0, (P0, 1)).astype(np.float32)


def simi_margins(points, centres, r):
    """float64: (nearest distance, relative gap to the second nearest, |d - r| / r) per point."""
    d = np.linalg.norm(points.astype(np.float64)[:, None, :] - centres.astype(np.float64)[None, :, :], axis=2)
    d.sort(axis=1)
    return d[:, 0], (d[:, 1] - d[:, 0]) / d[:, 0], np.abs(d[:, 0] - r) / r


@functools.lru_cache(maxsize=1)
def simi_points():
    """{voxel key: [k,3] float32 CPU tensor} with 257 points in all, around the centres of rows [100, 260), at 0.2 to 3
    times r = the mean scale of those rows, so some lie inside r (clamped to 0) and most outside.  Drawn in float64; a
    point whose two nearest centres differ by less than 1e-3 relative, or whose |d - r| < 1e-3 r, is drawn again."""
    sc = scene()
    lo, hi = SEL_ROWS
    centres, r = sc["means3D"][lo:hi], float(sc["scales"][lo:hi].astype(np.float64).mean())
    rng = np.random.default_rng(7)
    per_key = {k: [] for k in VOXEL_KEYS}
    n = 0
    while n < M_POINTS:
        j = int(rng.integers(0, hi - lo))
        u = rng.standard_normal(3)
        p = (centres[j].astype(np.float64) + u / np.linalg.norm(u) * r * rng.uniform(0.2, 3.0)).astype(np.float32)
        _, gap, clamp = simi_margins(p[None], centres, r)
        if gap[0] < MARGIN or clamp[0] < MARGIN:
            continue
        per_key[VOXEL_KEYS[j // 16]].append(p)
        n += 1
    return {k: torch.from_numpy(np.stack(v)) for k, v in per_key.items() if v}


def join_bar(terms):
    """J(s_1 .. s_n) per element; terms: float64 tensors of one shape."""
    return (len(terms) - 1) * EPS32 * sum(t.abs() for t in terms)


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class CheckFailed(AssertionError):
    """A property the session itself holds the host code to (raised before anything could run on stale state)."""


# ---- route A ---------------------------------------------------------------------------------------------------------
def _clone(t):
    return None if t is None else t.detach().clone()


class Session:
    """The product's loop on the device; `run()` returns the list of per-iteration records."""

    def __init__(self, dev):
        import gs_livm_amd as G
        self.G, self.dev = G, dev
        sc = scene()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        model = G.GrowableGaussians(1024, 4, dev)
        self.opt = G.GrowableAdam(model)
        xyz, scales = t(sc["means3D"]), t(sc["scales"])
        covs = torch.diag_embed(scales ** 2)
        rgbs = (torch.rand((P0, 3), generator=torch.Generator().manual_seed(4)) * 255).to(dev)
        lo, hi = SEL_ROWS
        assert model.add_new_pointcloud(xyz[:lo], covs[:lo], rgbs[:lo], 1.0) == (0, lo)
        assert model.add_new_pointcloud(xyz[lo:], covs[lo:], rgbs[lo:], 1.0, voxel_keys=VOXEL_KEYS + (REST_KEY,),
                                        voxel_counts=(16,) * 10 + (P0 - hi,)) == (lo, P0)
        with torch.no_grad():   # the leaves, in place: the scene's raw values
            model._xyz.copy_(xyz)
            model._scaling.copy_(torch.log(scales))
            o = t(sc["opacities"])
            model._opacity.copy_(torch.log(o / (1 - o)))
            model._rotation.copy_(t(sc["rotations"] * quat_factors()))
            model._features_dc.copy_(t(sc["shs"][:, :1]))
            model._features_rest.copy_(t(sc["shs"][:, 1:]))
        model.fused_tail = True
        model.enable_density_stats()
        self.vis = G.KeyframeVisibility(P0, device=dev)
        model.attach_visibility(self.vis)
        self.model = model
        self.cams = []
        for v, (rpy, T) in enumerate(POSES):
            cam = G.Camera(poses.rotation(**rpy), T, FOVX, FOVY, W, H, device=dev, uid=v)
            ref = cameras()[v]
            with torch.no_grad():   # poses.camera's own float32 arithmetic, so the oracle sees the same matrices
                cam._world_view_transform.copy_(t(ref["viewmatrix"]))
                cam._full_proj_transform.copy_(t(ref["projmatrix"]))
                cam._camera_center.copy_(t(ref["campos"]))
            self.cams.append(cam)
        self.bg = t(sc["bg"])
        self.masks = [m.to(dev) for m in keep_masks()]
        self.gts = [g.to(dev) for g in targets()]
        self.K = raster_K()
        self.iK = np.linalg.inv(self.K).astype(np.float32)
        pw = t(sweep())
        self.lidar = [G.lidar_depth_image(pw, G.world_to_camera(c), self.K, H, W) for c in self.cams]
        self.exposures = [torch.tensor(e, dtype=torch.float32, device=dev).requires_grad_(True) for e in EXPOSURES]
        self.xis = [torch.zeros(6, device=dev, requires_grad=True) for _ in self.cams]
        self.aux = torch.optim.Adam(self.exposures + self.xis, lr=1e-3)
        self.w = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in WEIGHTS.items()}
        self.select()

    def select(self):
        picked = self.model.voxel_index.select(simi_points(), max_points=10 ** 9)
        self.points, self.sel = picked

    def static(self):
        """What route B needs beside an iteration's record."""
        return dict(dev=self.dev, bg=self.bg, masks=self.masks, gts=self.gts, lidar=self.lidar, K=self.K, iK=self.iK,
                    w=self.w)

    @staticmethod
    def cam4(cam):
        return (cam.Get_world_view_transform(), cam.Get_projection_matrix(), cam.Get_full_proj_transform(),
                cam.Get_camera_center())

    def run(self):
        G, model = self.G, self.model
        G.set_binning_capacity_hint(0)           # forget the thread's history: the first forward is synchronous
        prev_nf = G.set_near_far_thread(False)   # one-chain frames: these tiny views must not feed the near-budget rule
        try:
            return [self._run_one(it) for it in range(1, ITERATIONS + 1)]
        finally:
            G.set_near_far_thread(prev_nf)

    def _run_one(self, it):
        G, model, w = self.G, self.model, self.w
        rec = dict(it=it, P=model.P)
        rec["leaves"] = {n: _clone(getattr(model, n)) for n in NAMES}
        rec["m"] = {n: _clone(model.moments(n)[0]) for n in NAMES}
        rec["v"] = {n: _clone(model.moments(n)[1]) for n in NAMES}
        rec["cams"] = [[_clone(x) for x in self.cam4(c)] for c in self.cams]
        rec["exposures"] = [_clone(e) for e in self.exposures]
        rec["next_act_in"] = None if model._next_act is None else [_clone(x) for x in model._next_act]
        rec["points"], rec["sel"] = self.points.clone(), self.sel.clone()
        rec["T_rel"] = [G.delta_pose(self.cams[s].Get_R(), self.cams[s].Get_T(), self.cams[r].Get_R(),
                                     self.cams[r].Get_T()) for s, r in PAIRS]
        spec0 = G.speculation_stats()["speculative_forwards"]
        # the iteration's first activated(): the similarity term's node, and the taker of _next_act
        _, opac, scales, rot, shs = model.activated()
        rec["act"] = [_clone(x) for x in (scales, rot, opac, shs)]
        views = []
        for ci in RENDERS:
            color, depth, acc, radii, m2d = G.render_full(self.cams[ci], model, self.bg, depth_gradient=True,
                                                          pose_tangent=self.xis[ci])
            for x in (color, depth, acc):
                x.retain_grad()
            mk = self.masks[ci]
            views.append(dict(color=color, depth=depth, acc=acc, radii=radii, m2d=m2d, cm=color * mk, dm=depth * mk,
                              am=acc * mk))
        rec["spec"] = G.speculation_stats()["speculative_forwards"] - spec0
        rec["images"] = [[_clone(v[k]) for k in ("color", "depth", "acc")] for v in views]
        rec["radii"] = [v["radii"].clone() for v in views]

        def alias(x):   # one consumer's own handle on a shared image: its .grad is that term's scaled gradient alone
            y = x.view_as(x)
            y.retain_grad()
            return y

        terms, taps = [], {}
        ex = self.exposures
        terms.append(("photo0", "photo", G.exposure_photometric_loss(views[0]["cm"], self.gts[0], ex[0], LAMBDAS["photo"])))
        terms.append(("photo1", "photo", G.exposure_photometric_loss(views[1]["cm"], self.gts[1], ex[1], LAMBDAS["photo"])))
        terms.append(("photo2", "photo", G.exposure_photometric_loss(views[2]["cm"], self.gts[2], ex[2], LAMBDAS["photo"],
                                                                     log_gain=True)))
        terms.append(("photo3", "photo", G.photometric_loss(views[3]["cm"], self.gts[0], LAMBDAS["photo"])))
        for v in range(3):
            d = taps["lidar%d.depth" % v] = alias(views[v]["dm"])
            terms.append(("lidar%d" % v, "lidar", G.lidar_depth_loss(d, views[v]["am"], self.lidar[v], ACC_MIN,
                                                                     LAMBDAS["lidar"])))
        for (s, r), T in zip(PAIRS, rec["T_rel"]):
            ds = taps["delta%d%d.src" % (s, r)] = alias(views[s]["dm"])
            dr = taps["delta%d%d.ref" % (s, r)] = alias(views[r]["dm"])
            terms.append(("delta%d%d" % (s, r), "delta", G.delta_depth_loss(ds, views[s]["am"], dr, views[r]["am"],
                                                                           self.iK, self.K.astype(np.float32), T,
                                                                           LAMBDAS["delta"])))
        terms.append(("simi", "simi", G.similarity_loss(self.points, self.sel, model._xyz, scales, LAMBDAS["simi"])))
        total = None
        for _, kind, term in terms:
            x = w[kind] * term                    # float32: the node's upstream is exactly float32(w)
            total = x if total is None else total + x
        total.backward()

        rec["total"] = _clone(total)
        rec["terms"] = {name: _clone(term) for name, _, term in terms}
        rec["parts"] = {name: _clone(term.grad_fn.parts) for name, _, term in terms}
        rec["image_grads"] = [[_clone(v[k].grad) for k in ("color", "depth", "acc")] for v in views]
        rec["taps"] = {k: _clone(x.grad) for k, x in taps.items()}
        rec["m2d_grads"] = [_clone(v["m2d"].grad) for v in views]
        rec["xyz_grad"] = _clone(model._xyz.grad)
        rec["act_grads"] = None if model._act_grads is None else [_clone(x) for x in model._act_grads]
        rec["exposure_grads"] = [_clone(e.grad) for e in ex]
        rec["xi_grads"] = [_clone(x.grad) for x in self.xis]
        rec["raw_grads_none"] = all(getattr(model, n).grad is None for n in NAMES[1:])

        for v in views:
            model.accumulate_density(v["radii"], v["m2d"].grad)
        rec["stats"] = _clone(model.density_stats())
        if it == 2:
            for v in views[:3]:
                self.vis.record(v["radii"])
            rec["vis"] = self.vis.bits.clone()
        rec["lrs"] = [next(g for g in self.opt.param_groups if any(q is getattr(model, n) for q in g["params"]))["lr"]
                      for n in NAMES]
        self.opt.step_model(model)
        rec["step"] = self.opt._step
        self.aux.step()
        self.aux.zero_grad(set_to_none=True)
        for cam, xi in zip(self.cams, self.xis):
            cam.retract(xi)
        rec["after"] = dict(leaves={n: _clone(getattr(model, n)) for n in NAMES},
                            m={n: _clone(model.moments(n)[0]) for n in NAMES},
                            v={n: _clone(model.moments(n)[1]) for n in NAMES},
                            next_act=None if model._next_act is None else [_clone(x) for x in model._next_act],
                            xyz_grad_cleared=model._xyz.grad is None, act_grads_cleared=model._act_grads is None,
                            exposures=[_clone(e) for e in ex], cams=[[_clone(x) for x in self.cam4(c)] for c in self.cams],
                            xis=[_clone(x) for x in self.xis])
        if it == 2:
            self._density_control(rec)
        return rec

    def _density_control(self, rec):
        """densify, then prune the rows no view of iteration 2 saw (and what the default thresholds drop)."""
        model = self.model
        P = model.P
        d = model.densify(DENSIFY["grad_threshold"], DENSIFY["size_threshold"], seed=5)
        if model._next_act is not None or model._act_grads is not None:
            raise CheckFailed("densify kept cached activations of the old row count")
        drop = torch.cat([self.vis.unobserved(1, P=P), torch.zeros(model.P - P, dtype=torch.uint8, device=self.dev)])
        p = model.prune(drop=drop)
        if model._next_act is not None or model._act_grads is not None:
            raise CheckFailed("prune kept cached activations of the old row count")
        self.select()
        rec["events"] = dict(densify={k: d[k] for k in ("P_before", "P_after", "n_new", "n_clone", "n_split")},
                             prune={k: p[k] for k in ("P_before", "P_after", "n_opacity", "n_scale", "n_nonfinite",
                                                      "n_mask")},
                             vis_rows=self.vis.rows, vis_bits=self.vis.bits.clone())


# ---- route B ---------------------------------------------------------------------------------------------------------
def replay(st, rec):
    """One iteration by hand from A's record; returns what `compare` holds against the record."""
    import gs_livm_amd as G
    from gs_livm_amd import _capi
    dev, w = st["dev"], st["w"]
    L = rec["leaves"]
    scales, rot, opac, shs = _capi.activate(L["_scaling"], L["_rotation"], L["_opacity"], L["_features_dc"],
                                            L["_features_rest"])
    xyz = L["_xyz"]
    empty = torch.empty(0, device=dev)
    tanx, tany = math.tan(FOVX * 0.5), math.tan(FOVY * 0.5)
    win = G.reference_window_1d().tolist()
    out = dict(act=[scales, rot, opac, shs], images=[], fwd=[])
    for ci in RENDERS:
        view, _, full, centre = rec["cams"][ci]
        f = _capi.rasterize_forward(st["bg"], xyz, empty, opac, scales, rot, 1.0, empty, view, full, tanx, tany, H, W,
                                    shs, 1, centre, False, False)
        out["fwd"].append(f)
        out["images"].append([f[1], f[2], f[3]])
    mk = [st["masks"][ci] for ci in RENDERS]
    cm = [(f[1] * m).contiguous() for f, m in zip(out["fwd"], mk)]
    dm = [(f[2] * m).contiguous() for f, m in zip(out["fwd"], mk)]
    am = [(f[3] * m).contiguous() for f, m in zip(out["fwd"], mk)]
    terms, color_g, acc_g, taps, exp_g = {}, [None] * 4, [None] * 4, {}, [None] * 3
    depth_terms = [[] for _ in range(4)]
    # photometric: views 0 and 1 per channel, view 2 shared log gain, render 3 plain
    for v in range(3):
        e = rec["exposures"][v]
        if v == 2:
            e = torch.stack((torch.exp(e[0]).expand(3), e[1].expand(3)), dim=1).contiguous()
        o3, g, ge = _capi.exposure_loss(cm[v], st["gts"][v], e, win, LAMBDAS["photo"])
        terms["photo%d" % v] = o3
        color_g[v] = (g * w["photo"]) * mk[v]
        ge = ge * w["photo"]
        if v < 2:
            exp_g[v] = ge
        else:   # d/da = sum_c ge[c,0] exp(a), d/db = sum_c ge[c,1]; float64, with the bar of its join
            a64 = rec["exposures"][2][0].double()
            t = torch.stack((ge[:, 0].double() * torch.exp(a64), ge[:, 1].double()), dim=1)      # [3 channels, 2]
            mag = t.abs().sum(0)
            exp_g[2] = (t.sum(0), 2 * EPS32 * mag + torch.tensor([2 * EPS32, 0.0], device=dev, dtype=torch.float64) * mag)
    o3, g = _capi.photometric_loss(cm[3], st["gts"][0], win, LAMBDAS["photo"])
    terms["photo3"] = o3
    color_g[3] = (g * w["photo"]) * mk[3]
    for v in range(3):
        o3, gd, ga = _capi.lidar_depth_loss(dm[v], am[v], st["lidar"][v], ACC_MIN, LAMBDAS["lidar"])
        terms["lidar%d" % v] = o3
        taps["lidar%d.depth" % v] = gd * w["lidar"]
        depth_terms[v].append(taps["lidar%d.depth" % v] * mk[v])
        acc_g[v] = (ga * w["lidar"]) * mk[v]
    for (s, r), T in zip(PAIRS, rec["T_rel"]):
        o3, _, gs, gr = _capi.delta_depth_loss(dm[s], am[s], dm[r], am[r], st["iK"], st["K"].astype(np.float32), T,
                                               LAMBDAS["delta"])
        terms["delta%d%d" % (s, r)] = o3
        taps["delta%d%d.src" % (s, r)] = gs * w["delta"]
        taps["delta%d%d.ref" % (s, r)] = gr * w["delta"]
        depth_terms[s].append(taps["delta%d%d.src" % (s, r)] * mk[s])
        depth_terms[r].append(taps["delta%d%d.ref" % (s, r)] * mk[r])
    gx, gsc = torch.zeros_like(xyz), torch.zeros_like(scales)
    terms["simi"] = _capi.similarity_loss(rec["points"], rec["sel"], xyz.contiguous(), scales, LAMBDAS["simi"], gx, gsc)
    gx, gsc = gx * w["simi"], gsc * w["simi"]
    out.update(terms=terms, color_g=color_g, acc_g=acc_g, taps=taps, exp_g=exp_g)
    out["depth_g"] = [(sum(t.double() for t in ts), join_bar([t.double() for t in ts])) if ts else None
                      for ts in depth_terms]
    out["total"] = sum(float(w[k.rstrip("0123456789")]) * float(terms[k][0].double()) for k in terms)
    out["total_mag"] = sum(abs(float(w[k.rstrip("0123456789")]) * float(terms[k][0].double())) for k in terms)
    # the four backwards, fed with A's retained image gradients
    per = dict(xyz=[], scales=[], rot=[], opac=[], shs=[])
    out["m2d"], pose = [], [[] for _ in range(3)]
    for r, ci in enumerate(RENDERS):
        view, _, full, centre = rec["cams"][ci]
        R, _, _, _, radii, geom, binning, img = out["fwd"][r]
        gc, gd, ga = rec["image_grads"][r]
        if ga is None:
            ga = torch.zeros((1, H, W), device=dev)
        b = _capi.rasterize_backward(st["bg"], xyz, radii, empty, scales, rot, 1.0, empty, view, full, tanx, tany, gc, ga,
                                     shs, 1, centre, geom, R, binning, img, False, return_conic=True, want_cov3D=False,
                                     grad_depth=gd)
        g_m2d, _, g_opac, g_m3d, _, g_sh, g_scales, g_rot, g_conic = b[:9]
        out["m2d"].append(g_m2d)
        pose[ci].append(_capi.pose_gradient(xyz, radii, scales, rot, 1.0, empty, view, full, tanx, tany, H, W, g_m2d,
                                            g_conic, g_m3d, b[9] if gd is not None else None))
        for k, g in zip(("xyz", "scales", "rot", "opac", "shs"), (g_m3d, g_scales, g_rot, g_opac, g_sh)):
            per[k].append(g.double())
    per["xyz"].append(gx.double())
    per["scales"].append(gsc.double())
    out["leaf_g"] = {k: (sum(ts), join_bar(ts)) for k, ts in per.items()}
    out["pose"] = pose
    # the step, on clones, from A's recorded gradients
    ps = [L[n].clone() for n in NAMES]
    ms = [rec["m"][n].clone() for n in NAMES]
    vs = [rec["v"][n].clone() for n in NAMES]
    if rec["xyz_grad"] is not None and rec["act_grads"] is not None:
        nxt = _capi.model_step(ps, ms, vs, rec["xyz_grad"].contiguous(), *rec["act_grads"], rec["lrs"], 0.9, 0.999,
                               1e-15, rec["step"])
        out["after"] = dict(leaves=dict(zip(NAMES, ps)), m=dict(zip(NAMES, ms)), v=dict(zip(NAMES, vs)), next_act=list(nxt))
    return out


# ---- A against B -------------------------------------------------------------------------------------------------------
def _ratio(got, want64, bar):
    err = (got.double() - want64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300))
    return float(r.max()) if r.numel() else 0.0


def compare(rec, B, prev=None):
    """{group: {check: ratio}} for one iteration: 0.0 / inf for an equality of bits, |d| / bar under a join bar.
    prev: the record of the iteration before (whose step left _next_act), or None."""
    inf = float("inf")
    eq = lambda a, b: 0.0 if same_bits(a, b) else inf  # noqa: E731
    res = {}
    g = res["forward"] = {}
    for i, name in enumerate(("scales", "rotations", "opacities", "shs")):
        g["activated." + name] = eq(rec["act"][i], B["act"][i])
    for r in range(4):
        for i, name in enumerate(("color", "depth", "acc")):
            g["render%d.%s" % (r, name)] = eq(rec["images"][r][i], B["images"][r][i])
        g["render%d.radii" % r] = eq(rec["radii"][r], B["fwd"][r][4])
    for k, o3 in B["terms"].items():
        g["term." + k] = eq(rec["terms"][k], o3[0])
        g["parts." + k] = eq(rec["parts"][k], o3)
    g["total"] = abs(float(rec["total"]) - B["total"]) / (len(B["terms"]) * EPS32 * B["total_mag"])
    if rec["it"] > 1 and prev is not None and "events" not in prev:
        for i, name in enumerate(("scales", "rotations", "opacities", "shs")):   # handed over, not recomputed
            g["next_act_in." + name] = eq(rec["next_act_in"][i] if rec["next_act_in"] else None, rec["act"][i])
    else:
        g["next_act_in.none"] = 0.0 if rec["next_act_in"] is None else inf

    g = res["image_grads"] = {}
    for r in range(4):
        g["render%d.color" % r] = eq(rec["image_grads"][r][0], B["color_g"][r])
        g["render%d.acc" % r] = eq(rec["image_grads"][r][2], B["acc_g"][r])
        want = B["depth_g"][r]
        got = rec["image_grads"][r][1]
        if want is None or got is None:
            g["render%d.depth" % r] = 0.0 if (want is None and got is None) else inf
        else:
            g["render%d.depth" % r] = _ratio(got, want[0], want[1])
    for k, t in B["taps"].items():
        g["term." + k] = eq(rec["taps"].get(k), t)

    g = res["leaf_grads"] = {}
    for r in range(4):
        g["render%d.means2D" % r] = eq(rec["m2d_grads"][r], B["m2d"][r])
    if rec["xyz_grad"] is None or rec["act_grads"] is None:
        g["parked"] = inf
    else:
        g["xyz"] = _ratio(rec["xyz_grad"], *B["leaf_g"]["xyz"])
        for i, k in enumerate(("scales", "rot", "opac", "shs")):
            g["act_grads." + k] = _ratio(rec["act_grads"][i], *B["leaf_g"][k])
    g["raw_leaf_grads_none"] = 0.0 if rec["raw_grads_none"] else inf
    for v in range(2):
        g["exposure%d" % v] = eq(rec["exposure_grads"][v], B["exp_g"][v])
    g["exposure2"] = inf if rec["exposure_grads"][2] is None else _ratio(rec["exposure_grads"][2], *B["exp_g"][2])
    for ci in (1, 2):
        g["pose%d" % ci] = eq(rec["xi_grads"][ci], B["pose"][ci][0])
    p0 = [t.double() for t in B["pose"][0]]
    g["pose0"] = inf if rec["xi_grads"][0] is None else _ratio(rec["xi_grads"][0], sum(p0), join_bar(p0))

    g = res["step"] = {}
    if "after" not in B:
        g["ran"] = inf
    else:
        A = rec["after"]
        for n in NAMES:
            g["leaf." + n] = eq(A["leaves"][n], B["after"]["leaves"][n])
            g["exp_avg." + n] = eq(A["m"][n], B["after"]["m"][n])
            g["exp_avg_sq." + n] = eq(A["v"][n], B["after"]["v"][n])
        for i, name in enumerate(("scales", "rotations", "opacities", "shs")):
            g["next_act." + name] = eq(A["next_act"][i] if A["next_act"] else None, B["after"]["next_act"][i])
        g["grads_cleared"] = 0.0 if (A["xyz_grad_cleared"] and A["act_grads_cleared"]) else inf
    return res


def flatten(records):
    """[(path, tensor or None)] of every tensor a session recorded, in a fixed order."""
    out = []

    def walk(path, x):
        if isinstance(x, dict):
            for k in sorted(x, key=str):
                walk(path + (str(k),), x[k])
        elif isinstance(x, (list, tuple)):
            for i, y in enumerate(x):
                walk(path + (str(i),), y)
        elif torch.is_tensor(x) or x is None:
            out.append((".".join(path), x))
        else:
            out.append((".".join(path), torch.tensor(float(x), dtype=torch.float64)))

    for rec in records:
        walk(("it%d" % rec["it"],), rec)
    return out


# ---- float64 anchor at the image level ---------------------------------------------------------------------------------
def image_anchor(st, rec, want_truth=False):
    """The composed image-level loss in float64 from the existing restatements, evaluated at A's own float32 images (so
    no stage inherits another's rounding): exposure_ref.truth / loss_ref.loss_parts for the photometric terms,
    lidar_ref.loss_ops, delta_ref.evaluate -- weights and keep mask included.  A's `total` and retained image gradients
    are held to  sum_k |w_k| bar_k  (each term's own bar from its module, max(2 e_ref, .) included)  +  the join bar of
    the sum  +  2^-23 of the magnitude for the products with float32(w).  A pixel leaves the comparison where a term's
    reference calls it fragile (lidar F3, delta F1-F3 and their taps): at most 1 % of a view, or `fragile` says so.
    Returns ({check: worst |d| / bar}, {view: fragile share}); with want_truth also {render: [float64 gradient of the
    colour, the depth, the silhouette image]} (a record without gradients is then enough: nothing is held).  CPU."""
    import delta_ref
    import exposure_ref
    import lidar_ref
    import loss_ref
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    w = {k: float(v) for k, v in st["w"].items()}                  # float32(w), widened
    win = loss_ref.reference_window_1d()
    masks = [cpu(st["masks"][ci]) for ci in RENDERS]
    imgs = [[cpu(x) for x in rec["images"][r]] for r in range(4)]
    cm = [imgs[r][0] * masks[r] for r in range(4)]
    dm = [(imgs[r][1] * masks[r])[0] for r in range(4)]
    am = [(imgs[r][2] * masks[r])[0] for r in range(4)]
    lam = LAMBDAS
    res, losses, loss_bars = {}, [], []
    truth = {r: [None, None, None] for r in range(4)}
    grads = rec.get("image_grads") or [[None] * 3] * 4
    exp_grads = rec.get("exposure_grads") or [None] * 3

    def hold(name, got, want, bar, keep=None):
        if name.startswith("render"):
            truth[int(name[6])][("color", "depth", "acc").index(name[8:])] = want
        if got is None:
            return
        err = (cpu(got).double().reshape(want.shape) - want).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300))
        if keep is not None:
            r = torch.where(keep, r, torch.zeros_like(r))
        res[name] = float(r.max())

    # photometric terms -> the colour gradients (one producer each) and the [3,2] exposure gradients
    for v in range(3):
        e = rec["exposures"][v]
        if v == 2:
            e = torch.stack((torch.exp(e[0]).expand(3), e[1].expand(3)), dim=1)     # on A's device: its own expf
        e = cpu(e).contiguous()
        t = exposure_ref.truth(cm[v], cpu(st["gts"][v]), e, win, lam["photo"])
        losses.append(w["photo"] * t["r64"]["loss"])
        loss_bars.append(w["photo"] * t["bar"]["loss"][1])
        want = masks[v].double() * w["photo"] * t["dimg"]
        hold("render%d.color" % v, grads[v][0], want, w["photo"] * t["bar_dimg"] + EPS32 * want.abs())
        dexp = w["photo"] * t["dexp"]
        bar_e = w["photo"] * t["bar_dexp"] + EPS32 * dexp.abs()
        if v < 2:
            hold("exposure%d" % v, exp_grads[v], dexp, bar_e)
        else:   # the shared leaf: d/da = sum_c g_c dL/dg_c, d/db = sum_c dL/db_c
            g = e[:, 0].double()
            terms = torch.stack((dexp[:, 0] * g, dexp[:, 1]), dim=1)
            bar = torch.stack((bar_e[:, 0] * g, bar_e[:, 1]), dim=1).sum(0) + 2 * EPS32 * terms.abs().sum(0) \
                + torch.tensor([EPS32, 0.0], dtype=torch.float64) * terms.abs().sum(0)
            hold("exposure2", exp_grads[2], terms.sum(0), bar)
    r64 = loss_ref.loss_parts(cm[3], cpu(st["gts"][0]), win, lam["photo"], torch.float64)
    r32 = loss_ref.loss_parts(cm[3], cpu(st["gts"][0]), win, lam["photo"], torch.float32)
    b = loss_ref.bars(r64, r32, loss_ref.floors(cm[3], cpu(st["gts"][0]), win, lam["photo"]))
    losses.append(w["photo"] * r64["loss"])
    loss_bars.append(w["photo"] * b["loss"][1])
    want = masks[3].double() * w["photo"] * r64["grad"]
    hold("render3.color", grads[3][0], want, w["photo"] * b["grad"][1] + EPS32 * want.abs())

    # depth terms -> the depth gradients (up to three consumers) and the silhouette gradients
    depth_terms = [[] for _ in range(3)]          # per view: (float64 gradient, bar, keep)
    fragile = [torch.zeros((H, W), dtype=torch.bool) for _ in range(3)]
    for v in range(3):
        zl = cpu(st["lidar"][v]).numpy()
        args = (dm[v].numpy(), am[v].numpy(), zl, ACC_MIN, lam["lidar"])
        t64, t32 = lidar_ref.loss_ops(*args), lidar_ref.loss_ops(*args, dtype=torch.float32)
        lb = lidar_ref.bars(dict(t64, depth=args[0], acc=args[1], lidar=zl, acc_min=ACC_MIN, lam=lam["lidar"]))
        bar = {k: torch.maximum(2 * (t32[k].double() - t64[k]).abs(), torch.as_tensor(lb["bar"][k], dtype=torch.float64))
               for k in ("loss", "grad_depth", "grad_acc")}
        fragile[v] |= lb["F3"]
        losses.append(w["lidar"] * float(t64["loss"]))
        loss_bars.append(w["lidar"] * float(bar["loss"]))
        depth_terms[v].append((w["lidar"] * t64["grad_depth"], w["lidar"] * bar["grad_depth"], ~lb["F3"]))
        want = masks[v][0].double() * w["lidar"] * t64["grad_acc"]
        hold("render%d.acc" % v, grads[v][2], want, w["lidar"] * bar["grad_acc"] + EPS32 * want.abs(), ~lb["F3"])
    for (s, r), T in zip(PAIRS, rec["T_rel"]):
        x = dict(depth_src=dm[s].numpy(), acc_src=am[s].numpy(), depth_ref=dm[r].numpy(), acc_ref=am[r].numpy(),
                 inv_K_src=st["iK"], K_ref=st["K"].astype(np.float32), T_rel=T.numpy(), lam=lam["delta"], H=H, W=W)
        ref = delta_ref.evaluate(x)
        losses.append(w["delta"] * float(ref["truth"]["loss"]))
        loss_bars.append(w["delta"] * float(ref["bar"]["loss"]))
        depth_terms[s].append((w["delta"] * ref["truth"]["grad_src"], w["delta"] * ref["bar"]["grad_src"],
                               ref["keep"]["grad_src"]))
        depth_terms[r].append((w["delta"] * ref["truth"]["grad_ref"], w["delta"] * ref["bar"]["grad_ref"],
                               ref["keep"]["grad_ref"]))
        fragile[s] |= ~ref["keep"]["grad_src"]
        fragile[r] |= ~ref["keep"]["grad_ref"]
    for v in range(3):
        terms = [masks[v][0].double() * t for t, _, _ in depth_terms[v]]
        bar = sum(b for _, b, _ in depth_terms[v]) + join_bar(terms) + EPS32 * sum(t.abs() for t in terms)
        keep = functools.reduce(lambda a, b: a & b, [k for _, _, k in depth_terms[v]])
        hold("render%d.depth" % v, grads[v][1], sum(terms), bar, keep)

    # the similarity term's value enters the total alone (its gradients meet the leaves: the leaf-level anchor)
    simi = float(rec["terms"]["simi"])
    n = len(losses) + 1
    mag = sum(abs(x) for x in losses) + abs(w["simi"] * simi)
    want_total = sum(losses) + w["simi"] * simi
    res["total"] = abs(float(rec["total"]) - want_total) / (sum(loss_bars) + (n - 1) * EPS32 * mag + EPS32 * mag)
    shares = {v: float(fragile[v].double().mean()) for v in range(3)}
    return (res, shares, truth) if want_truth else (res, shares)


# ---- float64 anchor at the leaves ------------------------------------------------------------------------------------
def leaf_anchor(st, rec):
    """The gradients that reach the leaves in float64: per render depth_ref.render64 of the scene built from A's recorded
    activated tensors and camera, on the oracle's frame of that scene, fed with A's retained image gradients (widened);
    summed over the four renders, plus the similarity term in float64 autograd (simi_ref) times float32(w).  Held against
    A's `_xyz.grad` and `_act_grads` (gradients with respect to the ACTIVATED tensors: no chain rule in between) at the
    sum of the per-render bounds of helpers.check_against_ref64 (the bound of a sum is the sum of the bounds), plus the
    join bar, plus the similarity term's bar of tests/test_gpu_simi.py's docstring, K 2^-23 magnitude with
    K = 9 + ceil(log2(max(3 n, m))).  Pose gradients: pose_ref.xi_gradient at pose_ref.bar + pushed_bar per render.
    Returns ({check: worst |d| / bar}, {render: rows the oracle and A disagree on}).  CPU; seconds."""
    import depth_ref
    import pose_ref
    import simi_ref
    from oracle import oracle as O
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    f32 = lambda t: np.ascontiguousarray(cpu(t).numpy(), dtype=np.float32)  # noqa: E731
    scales, rot, opac, shs = rec["act"]
    base = dict(scene(), means3D=f32(rec["leaves"]["_xyz"]), scales=f32(scales), rotations=f32(rot), opacities=f32(opac),
                shs=f32(shs))
    groups = dict(xyz="dL_dmeans3D", scales="dL_dscales", rot="dL_drotations", opac="dL_dopacity", shs="dL_dsh")
    terms = {k: [] for k in groups}
    bars = {k: 0.0 for k in groups}
    pose_want, pose_bar = [0.0] * 3, [0.0] * 3
    disagree = {}
    for r, ci in enumerate(RENDERS):
        view, _, full, centre = rec["cams"][ci]
        sc = dict(base, viewmatrix=f32(view), projmatrix=f32(full), campos=f32(centre))
        fr = O.forward(sc)
        disagree[r] = int((fr.radii != cpu(rec["radii"][r]).numpy()).sum())
        zero = np.zeros((1, H, W), np.float32)
        g_c, g_d, g_a = (zero if g is None else f32(g) for g in rec["image_grads"][r])
        ref = depth_ref.render64(sc, fr, g_c, g_a, g_d, slack=True)
        tol = pose_ref.group_tolerances(ref, tuple(groups.values()))
        for k, name in groups.items():
            terms[k].append(torch.from_numpy(np.asarray(ref[name], np.float64)))
            bars[k] = bars[k] + torch.from_numpy(np.array(tol[name], dtype=np.float64))
        vis = np.flatnonzero(fr.radii > 0)
        a = pose_ref.arrays_of(sc, fr.radii, ref)
        pose_want[ci] = pose_want[ci] + pose_ref.xi_gradient(sc, vis, fr.clamped, pose_ref.upstream2d(ref, vis))
        pose_bar[ci] = pose_bar[ci] + pose_ref.bar(a) + pose_ref.pushed_bar(a, pose_ref.group_tolerances(ref))
        fr.close()
    # the similarity term, float64 autograd on A's float32 inputs
    w = float(st["w"]["simi"])
    x = cpu(rec["leaves"]["_xyz"]).double().requires_grad_(True)
    s = cpu(scales).double().requires_grad_(True)
    pts, sel = cpu(rec["points"]).double(), cpu(rec["sel"])
    loss = simi_ref.similarity_loss_ref(pts, sel, x, s, LAMBDAS["simi"])
    gx, gs = torch.autograd.grad(loss, (x, s))
    terms["xyz"].append(w * gx)
    terms["scales"].append(w * gs)
    n, m = int(sel.numel()), int(pts.shape[0])
    K = 9 + math.ceil(math.log2(max(3 * n, m)))
    # magnitudes (test_gpu_simi): a row of the xyz gradient sums one vector of length lambda / m per point that shares it
    d = (pts[:, None, :] - x.detach()[sel.long()][None, :, :]).norm(dim=2)
    shares = torch.zeros(x.shape[0], dtype=torch.float64).index_add_(0, sel.long()[d.argmin(1)], torch.ones(m, dtype=torch.float64))
    bars["xyz"] = bars["xyz"] + w * K * EPS32 * (LAMBDAS["simi"] / m) * shares[:, None] + EPS32 * terms["xyz"][-1].abs()
    bars["scales"] = bars["scales"] + w * K * EPS32 * float(gs.abs().max()) * (gs != 0).double() + EPS32 * terms["scales"][-1].abs()
    res = {}

    def hold(name, got, ts, bar):
        want = sum(ts)
        err = (cpu(got).double().reshape(want.shape) - want).abs()
        bar = (bar + join_bar(ts)).reshape(want.shape)
        r_ = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300))
        res[name] = float(r_.max())

    hold("xyz", rec["xyz_grad"], terms["xyz"], bars["xyz"])
    for i, k in enumerate(("scales", "rot", "opac", "shs")):
        hold("act_grads." + k, rec["act_grads"][i], terms[k], bars[k])
    for ci in range(3):
        got = cpu(rec["xi_grads"][ci]).double().numpy()
        extra = EPS32 * np.abs(pose_want[ci]) if ci == 0 else 0.0           # camera 0: one float32 addition joins two renders
        res["pose%d" % ci] = float((np.abs(got - pose_want[ci]) / (pose_bar[ci] + extra)).max())
    return res, disagree
