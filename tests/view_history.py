"""Keyframe sessions against the per-view history (include/gsraster.h, "Per-view histories"): the scenes, the scripted
sessions and the per-frame check of tests/test_gpu_view_history.py; importable without a GPU (the scenes and scripts
are numpy only -- tests/test_view_history_cases.py holds them to the oracle).

A SESSION is a seeded script of frames and model changes through the surface the integration uses: Camera objects that
live for the whole session (the library keys a view's history by the address of its view matrix and the image size),
rasterize_forward + rasterize_backward, and a GrowableGaussians model changed between frames through its own API.  It
runs twice in one thread of a child process (run_session):
  reference pass  every frame synchronous and in one chain (near/far off for the thread, the history forgotten before
                  each forward); each distinct (model state, camera pose, image size) is rendered once and kept;
  natural pass    the history forgotten once, the thread's defaults restored, then NO hook for the rest of the session
                  (except where the script says "forget"): the frame kinds are whatever the library's own rules make of
                  the session.  New Camera objects, the same script.
Every frame of the natural pass -- four images, nine gradients, and gsr_backward_depth's ten on camera 0 -- is
bit-identical to its reference (int32 views, a NaN equals itself); the model states of both passes are identical
(every kernel of model.py's operations is bitwise reproducible), asserted once per state.  Some reference frames are
held to the CPU oracle with the parity suite's own check and bars (test_gpu_parity.check_forward, helpers.grad_close):
no tolerance is introduced here, every other comparison is exact.

Script operations (tuples):
  ("phase", name, lock_step)   what follows until the next phase; lock_step: torch.cuda.synchronize() after each frame
                               and the public read-outs taken; otherwise nothing waits and the mismatches are summed in
                               a device counter that is read at the end of the phase
  ("frame", cam, size, side)   forward then backward of camera `cam` at SIZES[size]; side: on the side stream
  ("round", cams, size)        all forwards, then all backwards (the reference's loop, lioOptimization.cpp:1691-1737)
  ("prune", tag)               model.prune(drop = rows tagged `tag`)     ("stack" or "grown")
  ("add_stack",)               the 64 stack splats appended              (add_new_pointcloud, leaves overwritten)
  ("grow", n, seed, opacity)   n large near splats appended              (likewise; opacity: large_splats' scale)
  ("densify", seed)            model.densify on statistics written by hand
  ("retract", cam, yaw_deg)    Camera.retract: the camera turns in place, its tensors keep their addresses
  ("forget",)                  gsr_set_binning_capacity_hint(0), natural pass only -- the one hook a script may ask for
  ("anchor",)                  the next new reference frame is held to the CPU oracle
"""
import json
import math
import os
import time

import numpy as np

from gs_livm_amd import synthetic as S

W, H = 320, 208                                     # 260 tiles
SIZES = ((320, 208), (160, 96), (640, 400))
P_BASE, SEED, N_STACK, N_GROW = 6000, 23, 64, 2400
FOVX_DEG = 60.0
NEAR_ENTRIES = 24                                   # GSR_NEAR_ENTRIES of the budget variants
TURN_DEG = 10.0                                     # the turn in place of the one-camera session
N_GROW_FAINT, FAINT = 3600, 0.2                     # the one-camera session's large splats: more and fainter
KEYS = ("means3D", "scales", "rotations", "opacities", "shs")
ENV_VARIANTS = {"near24": {"GSR_NEAR_ENTRIES": "24"},
                "near24-host-decided": {"GSR_NEAR_ENTRIES": "24", "GSR_ASYNC_FAR": "0"},
                "near24-partial-sort": {"GSR_NEAR_ENTRIES": "24", "GSR_PRE_HIST_MIN_P": "0"},
                "default": {}}


# ---- scenes (numpy) -------------------------------------------------------------------------------------------------
def stack_gaussians(P=P_BASE, seed=SEED):
    """test_gpu_parity._stack_scene's construction: N_STACK opaque screen-filling splats in front of the camera at yaw
    0 (rows 0 .. 63) over make_gaussians(P, seed).  At yaw 0 they finish every tile within a small near budget; seen
    from other yaws the stack leaves part of the image, whose tiles stay live."""
    g = S.make_gaussians(P, seed, sh_degree=0, aspect=W / H)
    g["means3D"][:N_STACK, :2] = 0.0
    g["means3D"][:N_STACK, 2] = np.linspace(0.5, 0.9, N_STACK, dtype=np.float32)
    g["scales"][:N_STACK] = 0.29
    g["opacities"][:N_STACK] = 0.98
    return g


def large_splats(n, seed, opacity_scale=1.0):
    """n large near splats: scale 0.25, z in [1, 1.5], xy x 0.2 -- each covers a good part of the image.  As drawn
    (opacity U(0.05, 0.95)) a default near budget of them finishes every tile; at opacity_scale FAINT it does not."""
    g = S.make_gaussians(n, seed, sh_degree=0, aspect=W / H)
    g["means3D"][:, :2] *= 0.2
    g["means3D"][:, 2] = np.random.default_rng(seed + 77).uniform(1.0, 1.5, n).astype(np.float32)
    g["scales"][:] = 0.25
    g["opacities"] *= np.float32(opacity_scale)
    return g


def rows(g, keep):
    return dict({k: g[k][keep] for k in KEYS}, sh_degree=0)


def cat(a, b):
    return dict({k: np.concatenate([a[k], b[k]]) for k in KEYS}, sh_degree=0)


def state_gaussians(name, P=P_BASE, n_grow=N_GROW, grow_seed=31, opacity_scale=1.0):
    """The scripted model states as numpy Gaussians: "stack", "pruned" (stack rows removed), "grown" (pruned + the large
    splats), "grown+stack" (the stack appended behind them, as the sessions put it back)."""
    base = stack_gaussians(P)
    if name == "stack":
        return base
    pruned = rows(base, np.arange(P) >= N_STACK)
    if name == "pruned":
        return pruned
    grown = cat(pruned, large_splats(n_grow, grow_seed, opacity_scale))
    if name == "grown":
        return grown
    assert name == "grown+stack", name
    return cat(grown, rows(base, np.arange(P) < N_STACK))


def camera(yaw_deg, Wc=W, Hc=H):
    """make_camera's camera for the BASE size's aspect (a Camera object keeps its matrices when its tensors are reused
    for another image size), with the image size of the frame."""
    c = S.make_camera(W, H, fovx_deg=FOVX_DEG, yaw_deg=float(yaw_deg))
    c["W"], c["H"] = int(Wc), int(Hc)
    return c


def scene_of(g, cam):
    return dict(g, **cam, bg=np.ones(3, np.float32), scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None)


def live_tiles_after_near(fr, entries_per_tile):
    """Tiles of the oracle frame `fr` (O.forward(..., tight=True)) that a near chain of `entries_per_tile` list entries
    per tile on average leaves unfinished, and the number of near Gaussians.  The near Gaussians are the prefix of the
    depth order (depth, then row: the order of the lists) whose instances fill the budget; a tile's near segment is the
    part of its list they make up -- a prefix, the list being depth-ordered.  A pixel is finished by it when it stopped
    reading its list inside the segment: its last contributor lies before the segment's end, and its transmittance
    there is below 1e-2 -- the stop test T (1 - alpha) < 1e-4 with alpha <= 0.99 (forward.cu:380-383) cannot fire
    above that, and an entry merely skipped for alpha < 1/255 is no stop."""
    T = fr.ranges.shape[0]
    budget = int(entries_per_tile) * T
    vis = np.nonzero(fr.radii > 0)[0]
    order = vis[np.lexsort((vis, fr.depths[vis]))]
    touched = fr.tiles_touched[order].astype(np.int64)
    near = np.zeros(fr.P, bool)
    near[order[np.cumsum(touched) - touched < budget]] = True
    gx = (fr.W + 15) // 16
    nc, fT = fr.n_contrib.reshape(fr.H, fr.W), fr.final_T.reshape(fr.H, fr.W)
    live = 0
    for t in range(T):
        lst = fr.point_list[fr.ranges[t, 0]:fr.ranges[t, 1]]
        in_near = near[lst]
        n_near = int(in_near.sum())
        assert in_near[:n_near].all()               # a prefix of the tile's list
        ty, tx = divmod(t, gx)
        px = (slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
        live += int(not ((nc[px] < n_near) & (fT[px] < 1e-2)).all())
    return live, int(near.sum())


# ---- scripts --------------------------------------------------------------------------------------------------------
def yaws_many(n=20):
    """n yaws in [-21, 21], cubically spaced and the smallest first: from most of them the stack still finishes every
    tile (up to 5 degrees, tests/test_view_history_cases.py), so a round opens with a long run of frames that
    speculate on their far chain and return without waiting -- many in flight -- and ends in misses."""
    y = 21.0 * np.linspace(-1.0, 1.0, n) ** 3
    return [float(v) for v in y[np.argsort(np.abs(y), kind="stable")]]


def script_one_camera(seed):
    """One camera at yaw 0, a changing model, in lock step (every outcome is resolved by the next forward)."""
    rng = np.random.default_rng(seed)
    grow_seed, densify_seed = int(rng.integers(1, 1 << 20)), int(rng.integers(1, 1 << 20))
    f = ("frame", 0, 0, False)
    ops = [("cameras", [0.0])]
    ops += [("phase", "stack", True), ("anchor",)] + [f] * 6        # ... until a frame speculates on its far chain
    # the camera turns in place by TURN_DEG: a few tiles stay live at the budget, none at one and a half budgets -- a
    # miss whose raise of the budget helps and is kept; and back
    ops += [("retract", 0, TURN_DEG), ("phase", "turned", True)] + [f] * 5
    ops += [("retract", 0, -TURN_DEG), ("phase", "turned back", True)] + [f] * 4
    ops += [("prune", "stack"), ("phase", "stack pruned", True), ("anchor",)] + [f] * 3   # a speculated miss; a raise
    # faint large splats: a capacity outgrown, a redo -- and tiles that stay live at the default budget too
    ops += [("grow", N_GROW_FAINT, grow_seed, FAINT), ("phase", "grown", True)] + [f] * 3
    ops += [("add_stack",), ("phase", "grown, stack back", True), ("anchor",)] + [f] * 5
    ops += [("prune", "stack"), ("phase", "stack pruned again", True)] + [f] * 2   # a miss at every budget
    ops += [("add_stack",), ("phase", "stack back again", True)] + [f] * 3
    ops += [("prune", "grown"), ("phase", "small again", True)] + [f] * 72   # the 64-frame rules
    ops += [("densify", densify_seed), ("phase", "densified", True), ("anchor",)] + [f] * 4
    ops += [("forget",), ("phase", "history forgotten", True)] + [f] * 4
    return ops


def script_many_cameras(seed, n_cams=40):
    """More cameras than view slots (32): three rounds of all forwards, then all backwards, nothing waiting in between;
    the model changes between the rounds.  The n_cams Camera objects stand at n_cams / 2 poses, two each -- the library
    tells views apart by their tensors, the reference frames are per pose."""
    rng = np.random.default_rng(seed)
    y = yaws_many(n_cams // 2)
    ops = [("cameras", [y[k % len(y)] for k in range(n_cams)])]
    ops += [("phase", "round 1: stack", False), ("anchor",), ("round", list(range(n_cams)), 0)]
    ops += [("prune", "stack"), ("phase", "round 2: stack pruned", False), ("anchor",),
            ("round", [int(k) for k in rng.permutation(n_cams)], 0)]
    ops += [("grow", N_GROW, int(rng.integers(1, 1 << 20)), 1.0), ("phase", "round 3: grown", False), ("anchor",),
            ("round", [int(k) for k in rng.permutation(n_cams)], 0)]
    return ops


def script_same_matrices(seed):
    """Two cameras whose tensors serve three image sizes in turn (the view key includes the size: each new size is a new
    view that inherits the most recent history); a camera that turns in place (same address, another frame); frames
    that alternate between the thread's default stream and a side stream without a host wait."""
    rng = np.random.default_rng(seed)
    ops = [("cameras", [0.0, 9.0])]
    for size in (0, 1, 2):
        ops += [("phase", "%dx%d" % SIZES[size], False)] + ([("anchor",)] if size == 0 else [])
        ops += [("frame", k & 1, size, False) for k in range(8)]
    ops += [("retract", 0, 20.0), ("phase", "camera 0 turned in place", False)]
    ops += [("frame", k & 1, 0, False) for k in range(6)]
    ops += [("prune", "stack"), ("phase", "alternating streams", False), ("anchor",)]
    ops += [("frame", k & 1, 0, bool(k & 1)) for k in range(8)]
    ops += [("grow", N_GROW, int(rng.integers(1, 1 << 20)), 1.0), ("phase", "alternating streams, grown", False),
            ("anchor",)]
    ops += [("frame", (k >> 1) & 1, 0, bool(k & 1)) for k in range(8)]
    return ops


SESSIONS = {"one_camera": script_one_camera, "many_cameras": script_many_cameras, "same_matrices": script_same_matrices}


def walk(script):
    """(frames, keys): every frame of the script as (frame index, camera, size, side stream, reference key, phase index,
    lock step), and the distinct reference keys in order of appearance.  A reference key is (model state, pose, size):
    the model state counts the model operations, the pose is (yaw the camera was made with, turns in place so far)."""
    state, poses, frames, keys, phase, lock = 0, [], [], [], -1, False
    for op in script:
        kind = op[0]
        if kind == "cameras":
            poses = [(round(float(y), 6), 0) for y in op[1]]
        elif kind == "phase":
            phase, lock = phase + 1, bool(op[2])
        elif kind in ("prune", "add_stack", "grow", "densify"):
            state += 1
        elif kind == "retract":
            poses[op[1]] = (poses[op[1]][0], poses[op[1]][1] + 1)
        elif kind in ("frame", "round"):
            shown = [(op[1], op[2], op[3])] if kind == "frame" else [(c, op[2], False) for c in op[1]]
            for cam, size, side in shown:
                key = (state, poses[cam], size)
                if key not in keys:
                    keys.append(key)
                frames.append((len(frames), cam, size, side, key, phase, lock))
        else:
            assert kind in ("forget", "anchor"), op
    return frames, keys


# ---- the session on the GPU -----------------------------------------------------------------------------------------
IMAGE_NAMES = ("color", "depth", "silhouette", "radii")
BWD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations", "dL_dconic")
COLS = IMAGE_NAMES + BWD_NAMES + tuple("depth:" + n for n in BWD_NAMES + ("dL_ddepths",))
DEPTH_CAM = 0                                       # the camera whose frames also run gsr_backward_depth


def _logit(o):
    o = o.astype(np.float64)
    return np.log(o / (1.0 - o)).astype(np.float32)


class _Pass:
    """One pass over a script: the model, the cameras and what both passes do alike."""

    def __init__(self, dev, script, refs):
        import torch
        import gs_livm_amd as G
        self.torch, self.G, self.dev, self.script = torch, G, dev, script
        self.refs, self.natural = refs, refs is not None and refs.get("complete", False)
        self.model = G.GrowableGaussians(1024, 1, dev)     # grows by doubling, as a map does
        self.tags = np.zeros(0, np.int8)                    # per row: 0 base, 1 stack, 2 grown, 3 densified
        self.state = 0
        self.bg = torch.ones(3, device=dev)
        self.empty = torch.empty(0, device=dev)
        self.cams, self.poses = [], []
        self.side = torch.cuda.Stream(device=dev)
        self.up = {}
        for size in range(len(SIZES)):
            self.upstream(size)
        base = stack_gaussians()
        self._append(rows(base, np.arange(P_BASE) < N_STACK), 1)
        self._append(rows(base, np.arange(P_BASE) >= N_STACK), 0)
        self._new_state(count=False)

    # -- model --
    def _append(self, g, tag):
        """Growth through add_new_pointcloud; the new rows' raw leaves are then overwritten in place with the chosen
        values (the leaves are views of the capacity buffers)."""
        torch, m = self.torch, self.model
        n = g["means3D"].shape[0]
        dev = self.dev
        lo, hi = m.add_new_pointcloud(torch.from_numpy(g["means3D"]).to(dev),
                                      (torch.eye(3, device=dev) * 1e-4).expand(n, 3, 3).contiguous(),
                                      torch.full((n, 3), 128.0, device=dev))
        assert hi - lo == n and hi == m.P
        with torch.no_grad():
            m._xyz[lo:hi] = torch.from_numpy(g["means3D"]).to(dev)
            m._features_dc[lo:hi] = torch.from_numpy(g["shs"][:, :1]).to(dev)
            m._scaling[lo:hi] = torch.from_numpy(np.log(g["scales"])).to(dev)
            m._rotation[lo:hi] = torch.from_numpy(g["rotations"]).to(dev)
            m._opacity[lo:hi] = torch.from_numpy(_logit(g["opacities"])).to(dev)
        self.tags = np.concatenate([self.tags, np.full(n, tag, np.int8)])

    def _new_state(self, count=True):
        torch, m = self.torch, self.model
        if count:
            self.state += 1
        assert m.P == len(self.tags)
        with torch.no_grad():
            self.act = tuple(x.detach() for x in m.activated())
        leaves = [getattr(m, n).detach() for n in m._NAMES]
        if not self.natural:
            self.refs.setdefault("leaves", {})[self.state] = [x.clone() for x in leaves]
        else:   # the same operations on the same values: the same model, bit for bit
            want = self.refs["leaves"][self.state]
            for n, a, b in zip(m._NAMES, leaves, want):
                assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (self.state, n)

    def model_op(self, op):
        torch, m = self.torch, self.model
        if op[0] == "prune":
            tag = {"stack": 1, "grown": 2}[op[1]]
            drop = torch.from_numpy(self.tags == tag).to(self.dev)
            out = m.prune(min_opacity=0.0, max_scale=float("inf"), drop=drop)
            assert out["P_before"] - out["P_after"] == int((self.tags == tag).sum()) == out["n_mask"] > 0, out
            self.tags = self.tags[self.tags != tag]
        elif op[0] == "add_stack":
            self._append(rows(stack_gaussians(), np.arange(P_BASE) < N_STACK), 1)
        elif op[0] == "grow":
            self._append(large_splats(op[1], op[2], op[3]), 2)
        else:   # densify on statistics written by hand, as test_densified_model_is_a_legal_model does
            assert op[0] == "densify", op
            m.enable_density_stats()
            gen = torch.Generator().manual_seed(op[1])
            m._stats[:m.P, 0] = torch.rand(m.P, generator=gen).to(self.dev)
            m._stats[:m.P, 1] = 1.0
            out = m.densify(0.9, 0.045, seed=op[1])
            assert out["n_clone"] > 20 and out["n_split"] > 20, out
            self.tags = np.concatenate([self.tags, np.full(out["n_new"], 3, np.int8)])
        self._new_state()

    # -- cameras --
    def make_cameras(self, yaws):
        G = self.G
        fovx = math.radians(FOVX_DEG)
        fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
        for k, yaw in enumerate(yaws):
            a = math.radians(yaw)
            R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
            self.cams.append(G.Camera(R, np.zeros(3, np.float32), fovx, fovy, W, H, device=self.dev, uid=k))
            self.poses.append((round(float(yaw), 6), 0))

    def retract(self, cam, yaw_deg):
        torch = self.torch
        xi = torch.zeros(6, device=self.dev)
        xi[4] = math.radians(yaw_deg)
        self.cams[cam].retract(xi)
        self.poses[cam] = (self.poses[cam][0], self.poses[cam][1] + 1)
        mats = [t.clone() for t in self._cam_tensors(self.cams[cam])]
        key = ("pose", self.poses[cam])
        if not self.natural:
            self.refs[key] = mats
        else:
            for a, b in zip(mats, self.refs[key]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key

    @staticmethod
    def _cam_tensors(cam):
        return cam.Get_world_view_transform(), cam.Get_full_proj_transform(), cam.Get_camera_center()

    # -- frames --
    def upstream(self, size):
        """fixed upstream images per size: make_upstream_grads, and a non-zero depth upstream of the same scale"""
        if size not in self.up:
            torch = self.torch
            Wc, Hc = SIZES[size]
            dcol, dacc = S.make_upstream_grads(Wc, Hc, 5)
            ddep = (np.random.default_rng(1000 + size).standard_normal((1, Hc, Wc)) / (Hc * Wc)).astype(np.float32)
            self.up[size] = tuple(torch.from_numpy(x).to(self.dev) for x in (dcol, dacc, ddep))
        return self.up[size]

    def _args(self, cam):
        c = self.cams[cam]
        view, full, center = self._cam_tensors(c)
        return view, full, center, math.tan(c.Get_FoVx() * 0.5), math.tan(c.Get_FoVy() * 0.5)

    def forward(self, cam, size):
        Wc, Hc = SIZES[size]
        view, full, center, tx, ty = self._args(cam)
        xyz, opac, scales, rot, shs = self.act
        return self.G.rasterize_forward(self.bg, xyz, self.empty, opac, scales, rot, 1.0, self.empty, view, full, tx,
                                        ty, Hc, Wc, shs, 0, center, False, False)

    def backward(self, cam, size, fwd, depth=False, upstream=None):
        view, full, center, tx, ty = self._args(cam)
        xyz, opac, scales, rot, shs = self.act
        dcol, dacc, ddep = upstream or self.upstream(size)
        return self.G.rasterize_backward(self.bg, xyz, fwd[4], self.empty, scales, rot, 1.0, self.empty, view, full,
                                         tx, ty, dcol, dacc, shs, 0, center, fwd[5], fwd[0], fwd[6], fwd[7], False,
                                         return_conic=True, grad_depth=ddep if depth else None)

    def oracle_scene(self, cam, size):
        Wc, Hc = SIZES[size]
        view, full, center, tx, ty = self._args(cam)
        xyz, opac, scales, rot, shs = (x.cpu().numpy() for x in self.act)
        return dict(means3D=xyz, opacities=opac, scales=scales, rotations=rot, shs=shs, sh_degree=0, W=Wc, H=Hc,
                    tanfovx=tx, tanfovy=ty, viewmatrix=view.cpu().numpy(), projmatrix=full.cpu().numpy(),
                    campos=center.cpu().numpy(), bg=np.ones(3, np.float32), scale_modifier=1.0, colors_precomp=None,
                    cov3D_precomp=None)


def reference_pass(dev, script):
    """-> refs: {key: dict(images, R, grads, depth_grads)}, the model leaves per state, the poses after each turn."""
    import torch
    import gs_livm_amd as G
    from helpers import grad_close
    from oracle import oracle as O
    from test_gpu_parity import GRAD_NAMES, check_forward, masked_grads
    refs = {"anchors": 0, "anchored_states": set()}
    p = _Pass(dev, script, refs)
    prev_nf = G.set_near_far_thread(False)
    anchor = False
    O.set_threads(min(O.max_threads(), 8))
    try:
        for op in script:
            kind = op[0]
            if kind == "cameras":
                p.make_cameras(op[1])
            elif kind in ("prune", "add_stack", "grow", "densify"):
                p.model_op(op)
            elif kind == "retract":
                p.retract(op[1], op[2])
            elif kind == "anchor":
                anchor = True
            elif kind in ("frame", "round"):
                shown = [(op[1], op[2])] if kind == "frame" else [(c, op[2]) for c in op[1]]
                for cam, size in shown:
                    key = (p.state, p.poses[cam], size)
                    if key in refs:
                        continue                                     # a state is rendered once
                    G.set_binning_capacity_hint(0)
                    fwd = p.forward(cam, size)                       # synchronous, one chain
                    assert not G.last_near_far()[0] and int(fwd[0]) == fwd[0].key == G.last_num_rendered()
                    g = p.backward(cam, size, fwd)
                    gd = p.backward(cam, size, fwd, depth=True) if cam == DEPTH_CAM else None
                    refs[key] = dict(images=fwd[1:5], R=int(fwd[0]), grads=g, depth_grads=gd)
                    if anchor:                                       # ... itself within tolerance of the oracle
                        anchor = False
                        sc = p.oracle_scene(cam, size)
                        fr = O.forward(sc, tight=True)
                        check_forward(sc, fr, fwd, dev, debug=False)
                        dc, da = masked_grads(sc["W"], sc["H"], 5, fr.fragile)
                        want = O.backward(fr, sc, dc, da)
                        got = p.backward(cam, size, fwd, upstream=(torch.from_numpy(dc).to(dev),
                                                                   torch.from_numpy(da).to(dev), None))
                        got = dict(zip(BWD_NAMES, (x.cpu().numpy() for x in got)))
                        for k in GRAD_NAMES:
                            grad_close(got[k], want[k], k)
                        refs["anchors"] += 1
                        refs["anchored_states"].add(p.state)
        torch.cuda.synchronize()
    finally:
        G.set_near_far_thread(prev_nf)
    refs["complete"] = True
    return refs


def _bits(x):
    import torch
    return x.view(torch.int32) if x.is_floating_point() else x


def natural_pass(dev, script, refs):
    """The script again, with new cameras and a new model, under the library's own rules.  -> the log: one record per
    frame (the public read-outs, lock-step phases only) and the counters before and after."""
    import torch
    import gs_livm_amd as G
    frames, _ = walk(script)
    p = _Pass(dev, script, refs)
    L = G.lib()
    bad = torch.zeros((len(frames), len(COLS)), dtype=torch.int32, device=dev)
    # forget the history once and restore the thread's defaults; from here on no hook
    G.set_near_far_thread(None)
    G.set_reference_rects_thread(None)
    G.set_near_far_hints(None, None)
    G.set_far_speculation(None)
    G.set_binning_capacity_hint(0)
    torch.cuda.synchronize()
    before = G.speculation_stats()
    log, checked = [], 0
    it = iter(frames)

    def compare(row, ref, fwd=None, g=None, gd=None):
        if fwd is not None:
            for j, (x, y) in enumerate(zip(ref["images"], fwd[1:5])):
                bad[row, j] = (_bits(x) != _bits(y)).sum()
        if g is not None:
            for j, (x, y) in enumerate(zip(ref["grads"], g)):
                bad[row, 4 + j] = (_bits(x) != _bits(y)).sum()
        if gd is not None:
            for j, (x, y) in enumerate(zip(ref["depth_grads"], gd)):
                bad[row, 13 + j] = (_bits(x) != _bits(y)).sum()

    def backwards(row, cam, size, ref, fwd):
        g = p.backward(cam, size, fwd)
        gd = p.backward(cam, size, fwd, depth=True) if cam == DEPTH_CAM else None
        compare(row, ref, g=g, gd=gd)

    def end_phase():
        nonlocal checked
        torch.cuda.synchronize()
        host = bad[checked:len(log)].cpu().numpy()
        if host.any():
            r, c = (int(v[0]) for v in np.nonzero(host))
            where = [(checked + int(i), frames[checked + int(i)][4]) for i in np.unique(np.nonzero(host)[0])[:8]]
            raise AssertionError("frame %d: %s differs from its reference in %d elements; frames that differ: %r; "
                                 "records: %s" % (checked + r, COLS[c], int(host[r, c]), where,
                                                  json.dumps(log[max(0, checked + r - 4):checked + r + 1])))
        checked = len(log)

    prev = dict(before)
    for op in script:
        kind = op[0]
        if kind == "cameras":
            p.make_cameras(op[1])
        elif kind == "phase":
            end_phase()
        elif kind in ("prune", "add_stack", "grow", "densify"):
            p.model_op(op)
        elif kind == "retract":
            p.retract(op[1], op[2])
        elif kind == "forget":
            G.set_binning_capacity_hint(0)
        elif kind == "frame":
            row, cam, size, side, key, phase, lock = next(it)
            ref = refs[key]
            stream = p.side if side else torch.cuda.current_stream()
            if side:
                p.side.wait_stream(torch.cuda.current_stream())     # (a stream-side wait: the host goes on)
            with torch.cuda.stream(stream):
                fwd = p.forward(cam, size)
                compare(row, ref, fwd=fwd)
                backwards(row, cam, size, ref, fwd)
            if side:
                torch.cuda.current_stream().wait_stream(p.side)
            rec = dict(frame=row, phase=phase, key_capacity=int(fwd[0].key))
            if lock:
                torch.cuda.synchronize()
                split, n_near, n_far = G.last_near_far()
                st = G.speculation_stats()
                rec.update(split=split, near=n_near, far=n_far, far_skipped=G.last_far_skipped(),
                           num_rendered=G.last_num_rendered(), scale=int(L.gsr_near_budget_scale()),
                           pause=int(L.gsr_near_far_pause(-1)), pending=G.async_outcomes_pending(),
                           **{k: st[k] - prev[k] for k in ("speculative_forwards", "overflows", "near_far_forwards",
                                                           "far_skips", "far_skip_misses", "async_far_frames",
                                                           "async_outcomes_lost")})
                prev = st
                # the instances this frame emitted: all of them in one chain, no more than that when it was split
                assert rec["num_rendered"] == n_near + n_far and rec["pending"] == 0, rec
                assert rec["num_rendered"] <= ref["R"] and (split or rec["num_rendered"] == ref["R"]), (rec, ref["R"])
            log.append(rec)
        elif kind == "round":
            held = []
            for cam in op[1]:                                        # all forwards, nothing waits in between
                row, cam_, size, side, key, phase, lock = next(it)
                fwd = p.forward(cam, size)
                compare(row, refs[key], fwd=fwd)
                held.append((row, cam, size, refs[key], fwd))
                log.append(dict(frame=row, phase=phase, key_capacity=int(fwd[0].key)))
            for row, cam, size, ref, fwd in held:                    # ... then all backwards
                backwards(row, cam, size, ref, fwd)
    end_phase()
    # (the counter can count: the last frame's reference against another model state's)
    last = frames[-1][4]
    others = [k for k in dict.fromkeys(f[4] for f in frames) if k[0] != last[0] and k[2] == last[2]]
    probe = torch.zeros(len(others), dtype=torch.int32, device=dev)
    for j, k in enumerate(others):
        probe[j] = sum((_bits(x) != _bits(y)).sum() for x, y in zip(refs[last]["images"][:3], refs[k]["images"][:3]))
    assert int(probe.max()) > 0
    torch.cuda.synchronize()
    pending = G.async_outcomes_pending()
    after = G.speculation_stats()
    delta = {k: after[k] - before[k] for k in before if k != "near_budget_scale_q8"}
    return dict(log=log, delta=delta, pending=pending, guard_trips=G.emit_guard_trips(), frames=len(frames))


def frame_kinds(log):
    """Per lock-step record: 'sync' (not speculative), 'one-chain', 'redo', 'split' (far chain enqueued outright),
    'hit' / 'miss' (speculated on its far chain)."""
    kinds = []
    for r in log:
        if "split" not in r:
            kinds.append(None)
        elif r["overflows"]:
            kinds.append("redo")
        elif r["far_skips"]:
            kinds.append("hit")
        elif r["far_skip_misses"]:
            kinds.append("miss")
        elif r["split"]:
            kinds.append("split")
        else:
            kinds.append("one-chain" if r["speculative_forwards"] else "sync")
    return kinds


def check_one_camera_kinds(script, log):
    """The frame kinds the lock-step session can derive from the documented rules and the observed outcomes, for the
    variants whose every speculative frame is split (a budget of NEAR_ENTRIES entries per tile).
    The rule (include/gsraster.h, "Far-chain speculation"): a split frame expects its far chain to stay idle exactly
    when the view's last two split frames left no quad unfinished.  Observed: a hit left none; a miss, a redo (its far
    chain outgrew its capacity) and a split frame whose far chain emitted instances left some.  At yaw 0 over a model
    that holds the stack nothing is left (tests/test_view_history_cases.py derives that from the oracle)."""
    frames, _ = walk(script)
    kinds = frame_kinds(log)
    names = [op[1] for op in script if op[0] == "phase"]
    with_stack = {i for i, n in enumerate(names) if n in ("stack", "turned back", "grown, stack back", "stack back again", "small again")}
    first = {}
    for i, f in enumerate(frames):
        first.setdefault(f[5], i)
    # the first phase: a synchronous frame, two split frames that leave nothing, and the third one speculates -- a hit
    i0 = first[names.index("stack")]
    assert kinds[i0:i0 + 4] == ["sync", "split", "split", "hit"], kinds[i0:i0 + 6]
    assert log[i0 + 3]["far_skipped"] and all(k == "hit" for k in kinds[i0 + 3:first[names.index("turned")]])
    # the camera turned in place under a streak: a speculated miss (a few tiles stay live: the cases test)
    it = first[names.index("turned")]
    assert kinds[it] == "miss" and not log[it]["far_skipped"] and log[it]["far"] > 0, (kinds[it], log[it])
    # the stack pruned under a streak: a speculated miss
    i1 = first[names.index("stack pruned")]
    assert kinds[i1] == "miss" and not log[i1]["far_skipped"] and log[i1]["far"] > 0, (kinds[i1], log[i1])
    # the model grown: the far chain outgrows the capacity its history gave it
    i2 = first[names.index("grown")]
    assert kinds[i2] == "redo", (kinds[i2], log[i2])
    # the rule, frame by frame: idle[k] of the split frames since the history was last forgotten
    i_forget = first[names.index("history forgotten")]
    idle = []
    for i, (k, r) in enumerate(zip(kinds, log)):
        if i == i_forget:
            idle = []                                # (a forgotten view starts from the thread's most recent history)
        if k in ("sync", "one-chain"):
            continue
        if len(idle) >= 2:                          # (a frame that speculated was scored: a hit or a miss)
            assert (r["far_skips"] + r["far_skip_misses"] == 1) == (idle[-1] and idle[-2]), (i, k, idle[-2:], r)
        if k in ("miss", "redo") or r["far"] > 0:
            idle.append(False)
        elif k == "hit" or r["phase"] in with_stack:
            idle.append(True)
        else:                                        # far chain enqueued outright, emitted nothing: cannot tell
            idle = []
    assert "hit" in kinds[i_forget:], kinds[i_forget:]
    # the adaptive near budget: the turn's misses raised it and the raise was kept (it finished the tiles); the pruned
    # stack's miss raised it on probation and the raise was taken back (nothing finishes there for lack of budget);
    # sixty-four frames in a row without a far chain then lower it by 16, once in the 75 such frames before the densify
    small = [r for r in log if r["phase"] == names.index("small again")]
    turned = [r for r in log if r["phase"] == names.index("turned")]
    pruned = [r for r in log if r["phase"] == names.index("stack pruned")]
    assert turned[0]["scale"] == 256 + 64 and turned[-1]["scale"] >= 256 + 64, [r["scale"] for r in turned]
    assert turned[-1]["far"] == 0 and kinds[first[names.index("turned back")] - 1] in ("split", "hit"), turned[-1]
    assert pruned[0]["scale"] == turned[-1]["scale"] + 64 and pruned[-1]["scale"] == turned[-1]["scale"], \
        [r["scale"] for r in pruned]
    assert small[0]["scale"] == turned[-1]["scale"] and small[-1]["scale"] == small[0]["scale"] - 16, \
        [r["scale"] for r in small]
    return kinds


def run_lengths(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def run_session(name, seed=7):
    """Both passes of one session in this process (a child of the test: GSR_NEAR_ENTRIES, GSR_ASYNC_FAR and
    GSR_PRE_HIST_MIN_P are read once per process, and the sessions' small frames must leave no history behind for the
    parent's later tests), then the conditions that make the run mean something, on the public read-outs only."""
    import torch
    dev = torch.device("cuda:0")
    near24 = os.environ.get("GSR_NEAR_ENTRIES") == str(NEAR_ENTRIES)
    use_async = os.environ.get("GSR_ASYNC_FAR", "1") != "0"
    script = SESSIONS[name](seed)
    frames, keys = walk(script)
    t0 = time.time()
    refs = reference_pass(dev, script)
    t1 = time.time()
    assert refs["anchors"] >= 3 and len(refs["anchored_states"]) >= 3, refs["anchors"]
    assert all(k in refs for k in keys)
    out = natural_pass(dev, script, refs)
    t2 = time.time()
    d, log = out["delta"], out["log"]
    summary = dict(session=name, near24=near24, use_async=use_async, frames=out["frames"], references=len(keys),
                   anchors=refs["anchors"], seconds_reference=round(t1 - t0, 2), seconds_natural=round(t2 - t1, 2),
                   delta=d, pending=out["pending"], guard_trips=out["guard_trips"])
    if name == "one_camera":
        summary["kinds"] = frame_kinds(log)
        summary["scales"] = run_lengths([r["scale"] for r in log])
        summary["pauses"] = sorted({r["pause"] for r in log})
        summary["capacities"] = run_lengths([r["key_capacity"] for r in log])
    print("SESSION " + json.dumps(summary), flush=True)
    assert d["frame_note_misses"] == 0 and out["pending"] == 0 and out["guard_trips"] == 0, summary
    speculated = d["far_skips"] + d["far_skip_misses"] + d["async_outcomes_lost"]
    if near24:      # three budgets are 18 720 instances, below the 65 536 floor of the prediction: every
        # speculative frame of these sizes is split
        assert 2 * d["near_far_forwards"] >= out["frames"], summary
        assert d["far_skips"] > 0 and d["far_skip_misses"] > 0, summary
        assert (d["async_far_frames"] > 0) == use_async, summary
    else:           # the default budget: one-chain capacity prediction, split frames only over the grown model
        assert 2 * d["speculative_forwards"] >= out["frames"], summary
        assert (d["async_far_frames"] > 0) == (use_async and speculated > 0), summary
    if use_async:   # every speculated frame's outcome was counted as a hit or a miss, or reported lost
        assert speculated == d["async_far_frames"], summary
    else:
        assert d["async_outcomes_lost"] == 0, summary
    if name == "one_camera":    # (over the grown model the default budget splits, speculates and misses as well)
        assert d["overflows"] >= 1 and d["far_skips"] > 0 and d["far_skip_misses"] > 0, summary
        assert any(r["scale"] != 256 for r in log), summary
        if near24:
            check_one_camera_kinds(script, log)
        else:   # one-chain frames: the capacity a view asked for last time is kept (a high-water mark) until the
            # prediction has been below half of it for 64 frames in a row -- within the 72 frames on the small state
            phase = [op[1] for op in script if op[0] == "phase"].index("small again")
            small = [r for r in log if r["phase"] == phase]
            assert frame_kinds(small)[8:] == ["one-chain"] * (len(small) - 8), summary
            assert small[-1]["key_capacity"] < small[8]["key_capacity"] // 2, summary
    print("session ok", flush=True)


if __name__ == "__main__":
    import sys
    run_session(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 7)
