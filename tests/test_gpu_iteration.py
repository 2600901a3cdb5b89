"""GPU tests of one whole optimiser iteration with every loss term at once (tests/iteration.py has the scene, the two
routes and the bars; DESIGN.md section 2, "One whole iteration", records the figures).

Route A is the product's loop through the public API, three iterations with densify and prune before the third; route
B replays each iteration by hand from A's records through the C ABI, summing in float64.  Every stage of B is pinned to
float64 by its own test file, so what these tests add is the composition: the `* g` of the five backward functions, the
depth image with up to three consumers, the gradients parked over five activation nodes, `_next_act` handed to the
next iteration and dropped by densify / prune, pose gradients of a camera rendered twice, the shared log-gain exposure,
four forwards' blobs alive before one backward.

Checks: equality of every bit where one producer feeds a tensor, the join bar J (tests/iteration.py) where autograd
adds.  Both routes run twice and every recorded tensor must repeat bit for bit.  Three float64 anchors at A's own
float32 values: the composed image-level loss of the reference modules (all iterations), the gradients at the leaves
and the pose gradients (iteration 1), and the step against tests/optim_ref.py, each at those modules' own bars.  Every
group prints its worst |d| / bar as a JSON line before it asserts.  `test_the_checks_see_host_mutants` breaks the host Python ten ways
(no kernel is touched) and demands that a check notices each; the table is profiles/iteration_mutants.txt.
"""
import functools
import json

import pytest
import torch

import gs_livm_amd as G
import iteration as I
import optim_ref
from gs_livm_amd import _capi
from gs_livm_amd import loss as GL
from gs_livm_amd import model as GM
from gs_livm_amd import rasterizer as GR

pytestmark = pytest.mark.gpu
GROUPS = ("forward", "image_grads", "leaf_grads", "step")


def _once(dev):
    """One session and its replay: (session, A's records, B's replays, {iteration: compare()})."""
    s = I.Session(dev)
    recs = s.run()
    torch.cuda.synchronize()
    st = s.static()
    Bs = [I.replay(st, rec) for rec in recs]
    res = {rec["it"]: I.compare(rec, b, recs[i - 1] if i else None) for i, (rec, b) in enumerate(zip(recs, Bs))}
    return s, recs, Bs, res


@functools.lru_cache(maxsize=1)
def _shared(dev_name):
    dev = torch.device(dev_name)
    a = I.Session(dev)
    recs_a = a.run()
    b = I.Session(dev)
    recs_b = b.run()                      # A twice before any of B's forwards: B stays out of A's view history
    torch.cuda.synchronize()
    st = a.static()
    B1 = [I.replay(st, rec) for rec in recs_a]
    B2 = [I.replay(st, rec) for rec in recs_a]
    res = {rec["it"]: I.compare(rec, x, recs_a[i - 1] if i else None) for i, (rec, x) in enumerate(zip(recs_a, B1))}
    return dict(session=a, recs=recs_a, recs_again=recs_b, B=B1, B_again=B2, res=res)


def test_the_session_runs_as_scripted(gpu_device):
    x = _shared(str(gpu_device))
    recs = x["recs"]
    print(json.dumps(dict(what="session", speculative_forwards=[r["spec"] for r in recs], rows=[r["P"] for r in recs],
                          events=recs[1]["events"]["densify"], prune=recs[1]["events"]["prune"],
                          total=[float(r["total"]) for r in recs])))
    st = recs[1]["stats"]
    seen = st[:, 1] > 0
    q = torch.quantile((st[seen, 0] / st[seen, 1]).double(), torch.tensor([0.1, 0.5, 0.9, 0.99], dtype=torch.float64,
                                                                         device=st.device))
    print(json.dumps(dict(what="density statistics after iteration 2", seen=int(seen.sum()),
                          mean_grad_quantiles=[float("%.3g" % v) for v in q])))
    assert recs[0]["spec"] == 3                                    # the hint: the session's first forward waits for its count
    assert recs[1]["spec"] == 4 and recs[2]["spec"] == 4           # every forward of iterations 2 and 3 speculates
    d, p = recs[1]["events"]["densify"], recs[1]["events"]["prune"]
    assert d["n_new"] > 0 and d["n_clone"] > 0 and d["n_split"] > 0 and d["P_after"] == I.P0 + d["n_new"]
    assert p["P_after"] < p["P_before"] and p["n_mask"] > 0 and p["n_scale"] > 0
    assert recs[2]["P"] == p["P_after"] != I.P0
    assert recs[1]["events"]["vis_rows"] == p["P_after"] and recs[1]["vis"].shape[0] == 3
    for r in recs:
        assert all(g is not None and bool(g.any()) for g in r["xi_grads"])
        assert all(g is not None and bool(g.any()) for g in r["exposure_grads"])
        assert r["image_grads"][3][1] is None and r["image_grads"][3][2] is None   # render 3: the colour alone
        assert all(bool(torch.isfinite(t).all()) for _, t in I.flatten([r]) if t is not None and t.is_floating_point())
    # the session trains: the leaves move at every step, and so do exposures and cameras
    for r in recs:
        for n in I.NAMES:
            assert not torch.equal(r["leaves"][n], r["after"]["leaves"][n]), n
        assert not torch.equal(r["cams"][1][0], r["after"]["cams"][1][0])
        assert not torch.equal(r["exposures"][2], r["after"]["exposures"][2])
        assert all(not bool(x.any()) for x in r["after"]["xis"])                   # retract zeroes the tangent


def test_a_second_run_reproduces_every_bit(gpu_device):
    x = _shared(str(gpu_device))
    a, b = I.flatten(x["recs"]), I.flatten(x["recs_again"])
    assert [k for k, _ in a] == [k for k, _ in b]
    diff = [k for (k, t), (_, u) in zip(a, b) if not I.same_bits(t, u)]
    print(json.dumps(dict(what="route A twice", tensors=len(a), different=diff[:10])))
    assert len(a) > 300 and not diff
    strip = lambda Bs: [{k: v for k, v in B.items() if k != "fwd"} for B in Bs]  # noqa: E731  (blobs hold padding)
    a, b = I.flatten([dict(B, it=i) for i, B in enumerate(strip(x["B"]))]), \
        I.flatten([dict(B, it=i) for i, B in enumerate(strip(x["B_again"]))])
    diff = [k for (k, t), (_, u) in zip(a, b) if not I.same_bits(t, u)]
    print(json.dumps(dict(what="route B twice", tensors=len(a), different=diff[:10])))
    assert len(a) > 150 and not diff


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("it", (1, 2, 3))
def test_the_product_equals_the_by_hand_route(it, group, gpu_device):
    res = _shared(str(gpu_device))["res"][it][group]
    worst = max(res, key=lambda k: res[k])
    joined = {k: float("%.4g" % v) for k, v in res.items() if 0.0 < v < float("inf")}
    print(json.dumps(dict(what="A against B", iteration=it, group=group, checks=len(res), worst=worst,
                          worst_over_bar=res[worst], join_bar_ratios=joined)))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad
    assert len(res) >= dict(forward=30, image_grads=19, leaf_grads=15, step=23)[group]


@pytest.mark.parametrize("it", (1, 2, 3))
def test_the_step_against_float64(it, gpu_device):
    """FusedAdam.step_model inside the loop against tests/optim_ref.py in float64, evaluated at A's own float32
    gradients, at that module's bars: the leaves, both moments and the activations handed to the next iteration."""
    rec = _shared(str(gpu_device))["recs"][it - 1]
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    names = dict(zip(optim_ref.GROUPS, I.NAMES))
    case = dict(P=rec["P"], M=4, p={k: cpu(rec["leaves"][n]) for k, n in names.items()},
                m={k: cpu(rec["m"][n]) for k, n in names.items()}, v={k: cpu(rec["v"][n]) for k, n in names.items()},
                ups=dict(xyz=cpu(rec["xyz_grad"]), scales=cpu(rec["act_grads"][0]), rotations=cpu(rec["act_grads"][1]),
                         opacities=cpu(rec["act_grads"][2]), shs=cpu(rec["act_grads"][3])))
    hyper = dict(step=rec["step"], eps=1e-15, lrs=[float(torch.tensor(x, dtype=torch.float32)) for x in rec["lrs"]])
    r64, r32 = optim_ref.model_step_ref(case, torch.float64, **hyper), optim_ref.model_step_ref(case, torch.float32, **hyper)
    ok = optim_ref.judgeable(case, r64, **hyper)
    dropped = optim_ref.dropped_fraction(ok)
    bar = optim_ref.bars(case, r64, r32, **hyper)
    A = rec["after"]
    got = dict(update={k: cpu(A["leaves"][n]).double() - case["p"][k].double() for k, n in names.items()},
               m={k: A["m"][n] for k, n in names.items()}, v={k: A["v"][n] for k, n in names.items()},
               next=dict(zip(optim_ref.ACTS, A["next_act"])), act=dict(zip(optim_ref.ACTS, rec["act"])))
    res = optim_ref.worst_ratios(got, r64, bar, ok)
    print(json.dumps(dict(what="step against float64", iteration=it, step=rec["step"], P=rec["P"], dropped=dropped,
                          worst_over_bar={k: float("%.4g" % v[3]) for k, v in res.items()})))
    assert rec["step"] == it and dropped <= optim_ref.DROP_CAP
    assert len(res) == 6 * 3 + 4 + 4
    assert max(v[3] for v in res.values()) <= 1.0, res


@pytest.mark.parametrize("it", (1, 2, 3))
def test_the_image_level_against_float64(it, gpu_device):
    """A's total and retained image gradients against the composed float64 loss of the reference modules
    (iteration.image_anchor), evaluated at A's own images."""
    x = _shared(str(gpu_device))
    res, fragile = I.image_anchor(x["session"].static(), x["recs"][it - 1])
    print(json.dumps(dict(what="image level against float64", iteration=it,
                          fragile_share={k: float("%.4g" % v) for k, v in fragile.items()},
                          worst_over_bar={k: float("%.4g" % v) for k, v in res.items()})))
    assert max(fragile.values()) <= 0.01
    assert len(res) == 4 + 3 + 3 + 3 + 1
    assert max(res.values()) <= 1.0, res


def test_the_leaf_level_against_float64(gpu_device):
    """What reaches the leaves in iteration 1 against depth_ref.render64 per render, summed, plus the similarity term
    and the pose gradients in float64 (iteration.leaf_anchor)."""
    x = _shared(str(gpu_device))
    res, disagree = I.leaf_anchor(x["session"].static(), x["recs"][0])
    print(json.dumps(dict(what="leaf level against float64", iteration=1, radii_disagree=disagree,
                          worst_over_bar={k: float("%.4g" % v) for k, v in res.items()})))
    assert not any(disagree.values())
    assert len(res) == 5 + 3
    assert max(res.values()) <= 1.0, res


# ---- mutants of the host Python ------------------------------------------------------------------------------------------
def _lidar_no_g(ctx, g):
    return ctx.grads[0], ctx.grads[1], None, None, None


def _delta_no_g(ctx, g):
    return ctx.grads[0], None, ctx.grads[1], None, None, None, None, None


def _delta_swapped(ctx, g):
    gs, gr = ctx.grads
    return gr * g, None, gs * g, None, None, None, None, None


def _simi_no_g(ctx, g):
    return None, None, ctx.grads[0], ctx.grads[1], None


def _stash_replaces(ctx, g_scales, g_rot, g_opac, g_shs):
    m = ctx.model
    new = [g_scales, g_rot, g_opac, g_shs]
    shapes = [m._scaling.shape, m._rotation.shape, m._opacity.shape, (m._xyz.shape[0], 1 + m._features_rest.shape[1], 3)]
    m._act_grads = [torch.zeros(sh, device=m._xyz.device) if g is None else g.contiguous() for g, sh in zip(new, shapes)]
    return None, None, None, None, None, None


def _raster_backward(ignore_depth=False, always_ddepth=False):
    """_RasterizeGaussians.backward, restated with one of two faults."""
    def backward(ctx, grad_color, _grad_radii, _grad_depth, grad_acc):
        s = ctx.settings
        grad_depth = None if ignore_depth else (_grad_depth if s.depth_gradient else None)
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img = ctx.saved_tensors
        if grad_color is None:
            grad_color = torch.zeros((3, s.image_height, s.image_width), device=means3D.device)
        if grad_acc is None:
            grad_acc = torch.zeros((1, s.image_height, s.image_width), device=means3D.device)
        want_pose = ctx.with_pose and ctx.needs_input_grad[9]
        out = _capi.rasterize_backward(
            s.bg, means3D.contiguous(), radii, colors_precomp.contiguous(), scales.contiguous(), rotations.contiguous(),
            s.scale_modifier, cov3Ds_precomp.contiguous(), s.viewmatrix.contiguous(), s.projmatrix.contiguous(), s.tanfovx,
            s.tanfovy, grad_color, grad_acc, sh.contiguous(), s.sh_degree, s.camera_center.contiguous(), geom,
            ctx.num_rendered, binning, img, False, return_conic=want_pose, want_cov3D=cov3Ds_precomp.numel() != 0,
            grad_depth=grad_depth)
        g_means2D, g_colors, g_opac, g_means3D, g_cov3D, g_sh, g_scales, g_rot = out[:8]
        g_pose = None
        if want_pose:
            ddepths = out[9] if (always_ddepth and s.depth_gradient) or grad_depth is not None else None
            g_pose = _capi.pose_gradient(means3D.contiguous(), radii, scales.contiguous(), rotations.contiguous(),
                                         s.scale_modifier, cov3Ds_precomp.contiguous(), s.viewmatrix.contiguous(),
                                         s.projmatrix.contiguous(), s.tanfovx, s.tanfovy, s.image_height, s.image_width,
                                         g_means2D, out[8], g_means3D, ddepths)
        return (g_means3D, g_means2D, g_sh, None, g_opac, g_scales, g_rot, None, None, g_pose)
    return backward


GM_STEP = GM.FusedAdam.step_model                                  # (the unbroken one, taken before any patch)


@torch.no_grad()
def _step_model_keeps_xyz_grad(self, model):
    grad = model._xyz.grad
    GM_STEP(self, model)
    model._xyz.grad = grad


def _bind_keeps_next_act(self):
    for name in self._NAMES:
        setattr(self, name, torch.nn.Parameter(self._buf[name][:self.P]))
    self._act_grads = None
    if self._optimizer is not None:
        self._optimizer.rebind(self)


def _per_channel_without_exp(exposure, channels, log_gain=False):
    if exposure.dim() == 1:
        exposure = exposure.expand(channels, 2)
    return exposure


MUTANTS = (
    ("LidarDepthLoss.backward without * g", GL.LidarDepthLoss, "backward", staticmethod(_lidar_no_g)),
    ("DeltaDepthLoss.backward without * g", GL.DeltaDepthLoss, "backward", staticmethod(_delta_no_g)),
    ("SimilarityLoss.backward without * g", GL.SimilarityLoss, "backward", staticmethod(_simi_no_g)),
    ("_StashingActivations.backward replaces _act_grads", GM._StashingActivations, "backward", staticmethod(_stash_replaces)),
    ("_RasterizeGaussians.backward ignores _grad_depth", GR._RasterizeGaussians, "backward",
     staticmethod(_raster_backward(ignore_depth=True))),
    ("_RasterizeGaussians.backward passes out[9] without a depth gradient", GR._RasterizeGaussians, "backward",
     staticmethod(_raster_backward(always_ddepth=True))),
    ("step_model leaves _xyz.grad in place", GM.FusedAdam, "step_model", _step_model_keeps_xyz_grad),
    ("_bind keeps _next_act", GM.GrowableGaussians, "_bind", _bind_keeps_next_act),
    ("_per_channel drops exp for log_gain", GL, "_per_channel", _per_channel_without_exp),
    ("DeltaDepthLoss.backward swaps gs and gr", GL.DeltaDepthLoss, "backward", staticmethod(_delta_swapped)),
)


def _failing(dev):
    """The A-against-B checks that fail on a fresh session, or the host-side exception that ended it."""
    try:
        _, _, _, res = _once(dev)
    except (I.CheckFailed, IndexError) as e:
        return ["session stopped: %s: %s" % (type(e).__name__, e)]
    return ["it%d.%s.%s" % (it, grp, k) for it in sorted(res) for grp in GROUPS for k, v in res[it][grp].items()
            if not v <= 1.0]


def test_the_checks_see_host_mutants(gpu_device, monkeypatch):
    """Each mutant changes host Python only (no kernel is touched, and the session stops on its own check before stale
    shapes could reach one); each must fail at least one A-against-B check, and the unbroken code none."""
    assert _failing(gpu_device) == []
    rows = []
    for name, owner, attr, fn in MUTANTS:
        with monkeypatch.context() as mp:
            mp.setattr(owner, attr, fn)
            failing = _failing(gpu_device)
        rows.append((name, failing))
        print(json.dumps(dict(what="mutant", mutant=name, caught=bool(failing), failing_checks=len(failing),
                              first=failing[:4])))
    assert _failing(gpu_device) == []                              # the patches are gone
    missed = [name for name, failing in rows if not failing]
    assert not missed, missed
