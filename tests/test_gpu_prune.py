"""GPU tests of in-place pruning (csrc/prune.hip through gsr_prune_mark / gsr_prune_compact, GrowableGaussians.prune):
every comparison is exact -- the rule against tests/prune_ref.py on the outputs of `_capi.activate`, the compaction
against t[keep], the pruned model against a model rebuilt from t[keep], renders before against renders after."""
import ctypes as C

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import prune_ref as R
from arena import PAT, Arena, offsets

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
LRS = dict(position_lr=0.0005, feature_lr=0.001, opacity_lr=0.025, scaling_lr=0.0025, rotation_lr=0.0025)


def _leaves(P, M, dev, seed=0):
    """raw leaves that all survive the default rule (scales ~ e^-3, opacities around 0.5)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    return {"_xyz": r(P, 3), "_features_dc": r(P, 1, 3), "_features_rest": r(P, M - 1, 3) * 0.1,
            "_scaling": r(P, 3) * 0.3 - 3.0, "_rotation": r(P, 4), "_opacity": r(P, 1)}


def _apply_pattern(L, pattern, seed):
    """makes rows dead by the RULE (huge scale or tiny opacity, alternately) so that keep follows `pattern`"""
    P = L["_xyz"].shape[0]
    i = torch.arange(P)
    g = torch.Generator().manual_seed(seed)
    if pattern == "all":
        dead = torch.zeros(P, dtype=torch.bool)
    elif pattern == "none":
        dead = torch.ones(P, dtype=torch.bool)
    elif pattern == "first":
        dead = i != 0
    elif pattern == "last":
        dead = i != P - 1
    elif pattern == "alternating":
        dead = i % 2 == 1
    elif pattern == "runs300":          # runs of 300: their ends fall inside workgroups (256 rows) and cross their seams
        dead = (i // 300) % 2 == 1
    else:
        dead = torch.rand(P, generator=g) >= float(pattern)   # pattern = share kept
    dead = dead.to(L["_xyz"].device)
    by_scale = dead & (torch.arange(P, device=dead.device) % 2 == 0)
    L["_scaling"][by_scale, 1] = 0.5          # exp = 1.65 > 0.3
    L["_opacity"][dead & ~by_scale] = -9.0    # sigmoid = 1.2e-4 < 1/255
    return ~dead


def _reference(L, drop_nonfinite=True, drop=None, lo=R.MIN_OPACITY, hi=R.MAX_SCALE):
    scales, _, opac, _ = _capi.activate(L["_scaling"], L["_rotation"], L["_opacity"], L["_features_dc"],
                                        L["_features_rest"])
    raw = [L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"]]
    return R.reasons_ref(opac, scales, raw=raw, min_opacity=lo, max_scale=hi, drop_nonfinite=drop_nonfinite, drop=drop)


def _mark(L, **kw):
    return _capi.prune_mark(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], **kw)


def _check_mark(L, lo=R.MIN_OPACITY, hi=R.MAX_SCALE, drop_nonfinite=True, drop=None):
    reasons, row_map, counts = _mark(L, min_opacity=lo, max_scale=hi, drop_nonfinite=drop_nonfinite, drop=drop)
    ref = _reference(L, drop_nonfinite=drop_nonfinite, drop=drop, lo=lo, hi=hi)
    assert torch.equal(reasons, ref)
    assert torch.equal(row_map, R.row_map_ref(ref))
    assert counts.tolist() == R.counts_ref(ref)
    return reasons, row_map, counts


# 300 007 rows are 1 172 workgroups: k_prune_scan's loop takes 1 024 workgroup totals per pass, so this size runs the
# loop twice -- a full pass, the carry into the next, and a partial last pass (148 totals, the last thread's four items
# cut short) -- and its strided reason sums take five rounds.  That is every level and loop the scan has.
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 300_007)
PATTERNS = ("all", "none", "first", "last", "alternating", "runs300", "0.03", "0.5", "0.97")


@pytest.mark.parametrize("P", SIZES)
def test_mark_matches_the_rule_on_the_activated_values(P, gpu_device):
    for n, pattern in enumerate(PATTERNS):
        L = _leaves(P, 1, gpu_device, seed=P + n)
        keep = _apply_pattern(L, pattern, seed=n)
        reasons, row_map, counts = _check_mark(L)
        assert torch.equal(reasons == 0, keep), pattern
        assert int(row_map[P]) == int(keep.sum()) == int(counts[0])


def test_mark_boundaries_nonfinite_and_caller_mask(gpu_device):
    dev, P = gpu_device, 1000
    L = _leaves(P, 1, dev, seed=3)
    # Thresholds that ARE activated values: row 10's opacity, a row's largest scale.  On the threshold = kept (the
    # rasterizer culls on >); with the threshold moved by ONE float the same row is one float beyond it and is dropped.
    scales, _, opac, _ = _capi.activate(L["_scaling"], L["_rotation"], L["_opacity"], L["_features_dc"], L["_features_rest"])
    lo = float(opac[10, 0])
    lo_up = float(np.nextafter(np.float32(lo), np.float32(1)))
    for k in range(3):                                                   # each of the three scale components in turn
        row = int((scales.argmax(1) == k).nonzero()[0])                  # a row whose largest scale is component k
        hi = float(scales[row, k])
        hi_down = float(np.nextafter(np.float32(hi), np.float32(0)))
        r = _check_mark(L, lo=lo, hi=hi)[0]
        assert int(r[10]) & R.OPACITY == 0 and int(r[row]) & R.SCALE == 0
        assert 0 < int((r & R.OPACITY).ne(0).sum()) < P and 0 < int((r & R.SCALE).ne(0).sum()) < P
        assert int(_check_mark(L, lo=lo, hi=hi_down)[0][row]) & R.SCALE  # one float above the threshold
    assert int(_check_mark(L, lo=lo_up, hi=hi)[0][10]) & R.OPACITY       # one float below the threshold
    # NaN and +-Inf in each of the four checked tensors, with the third bit on and off
    L = _leaves(P, 1, dev, seed=4)
    row = 30
    for name in ("_xyz", "_scaling", "_rotation", "_opacity"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            L[name].view(P, -1)[row, -1] = bad
            row += 37
    on = _check_mark(L, drop_nonfinite=True)[0]
    off = _check_mark(L, drop_nonfinite=False)[0]
    assert int((on & R.NONFINITE).ne(0).sum()) == 12 and not (off & R.NONFINITE).any()
    nan_rows = torch.isnan(L["_opacity"].view(-1)) | torch.isnan(L["_scaling"]).any(1)
    assert int(nan_rows.sum()) == 2 and not off[nan_rows].any()   # a NaN passes both comparisons: only the third bit catches it
    # the caller's mask alone (nothing else drops), and together with the rule (bool and uint8 masks)
    L = _leaves(P, 1, dev, seed=5)
    mask = torch.rand(P, device=dev) < 0.3
    r = _check_mark(L, drop=mask)[0]
    assert torch.equal(r, mask.to(torch.uint8) * R.MASK)
    _apply_pattern(L, "0.5", seed=2)
    r = _check_mark(L, drop=mask.to(torch.uint8) * 7)[0]
    assert bool(((r & R.MASK) != 0).eq(mask).all()) and int((r == (R.MASK | R.OPACITY)).sum()) > 0
    # P == 0: a no-op that yields P' = 0
    E = _leaves(0, 1, dev)
    reasons, row_map, counts = _mark(E)
    assert reasons.numel() == 0 and row_map.tolist() == [0] and counts.tolist() == [0, 0, 0, 0, 0]


def _eighteen(P, M, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    shapes = {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (M - 1, 3), "_scaling": (3,), "_rotation": (4,),
              "_opacity": (1,)}
    return {k + n: torch.randn((P,) + s, generator=gen).to(dev) for n, s in shapes.items() for k in ("p.", "m.", "v.")}


def _compact_in_arena(src, reasons, row_map, P_new, dev, mode, extra_rows=5):
    """sources AND destinations as guarded views at the byte offsets of `mode`; destinations have extra_rows rows more
    than P', prefilled with the NaN pattern.  Returns the destinations (views) after the launch."""
    ar = Arena(dev, offsets(mode))
    s = [ar.put("s." + k, src=t) for k, t in src.items()]
    d = [ar.put("d." + k, shape=(P_new + extra_rows,) + tuple(t.shape[1:])) for k, t in src.items()]
    _capi.prune_compact(s, d, reasons, row_map)
    torch.cuda.synchronize()
    assert ar.guards_intact() is None
    for t_src, t_in in zip(src.values(), s):
        assert torch.equal(t_src, t_in)                  # the sources are only read
    return d


@pytest.mark.parametrize("M", [1, 4, 16])
def test_compact_moves_all_eighteen_tensors(M, gpu_device):
    dev, P = gpu_device, 4097 + 300
    src = _eighteen(P, M, dev, seed=M)
    for pattern in ("0.5", "runs300", "all", "none", "first", "last", "0.97"):
        L = _leaves(P, 1, dev, seed=1)
        keep = _apply_pattern(L, pattern, seed=M)
        reasons, row_map, counts = _mark(L)
        P_new = int(counts[0])
        assert P_new == {"all": P, "none": 0}.get(pattern, P_new)       # P' = P and P' = 0 are among the cases
        want = R.compact_ref(list(src.values()), reasons)
        base = _compact_in_arena(src, reasons, row_map, P_new, dev, "a0")
        for (name, t), got, ref in zip(src.items(), base, want):
            assert torch.equal(got[:P_new], ref), (name, pattern)        # bit for bit t[keep]
            if got[P_new:].numel():                                      # rows [P', ...) exactly as they were filled
                assert bool((got[P_new:].view(torch.int32) == PAT).all()), (name, pattern)
        if pattern in ("0.5", "runs300"):
            # every offset the contract permits (4-byte element alignment) gives the aligned run's bits
            for mode in ("a4", "a8", "a12", "mix"):
                for got, ref in zip(_compact_in_arena(src, reasons, row_map, P_new, dev, mode), base):
                    assert torch.equal(got[:P_new], ref[:P_new]), (mode, pattern)
    # the free function for callers who hold plain tensors
    outs = G.prune_rows(list(src.values()), reasons, row_map, P_new)
    for got, ref in zip(outs, want):
        assert got.shape == ref.shape and torch.equal(got, ref)


def test_compact_refuses_the_offsets_the_contract_forbids(gpu_device):
    """Anything that is not a multiple of 4 bytes is refused before a launch; the destination keeps its fill."""
    dev, P = gpu_device, 300
    L = _leaves(P, 1, dev)
    _apply_pattern(L, "0.5", seed=0)
    reasons, row_map, counts = _mark(L)
    src = torch.randn((P + 1, 3), device=dev)
    dst = torch.full((P + 1, 3), 7.0, device=dev)
    VP = C.c_void_p * 1
    w = (C.c_int * 1)(3)
    lib = G.lib()
    for off in (1, 2, 3):
        for s_off, d_off in ((off, 0), (0, off)):
            code = lib.gsr_prune_compact(P, 1, VP(src.data_ptr() + s_off), VP(dst.data_ptr() + d_off), w,
                                         C.c_void_p(reasons.data_ptr()), C.c_void_p(row_map.data_ptr()), None)
            assert code == -1 and b"misaligned" in lib.gsr_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())


# ---- the model ------------------------------------------------------------------------------------------------------
def _model(leaves, moments, dev, step=0, capacity=None, voxels=None):
    """a GrowableGaussians + GrowableAdam holding the given rows (and moments, step count, voxel index)"""
    P, M = leaves["_xyz"].shape[0], 1 + leaves["_features_rest"].shape[1]
    m = G.GrowableGaussians(capacity or P + 64, M, dev)
    for n in NAMES:
        m._buf[n][:P].copy_(leaves[n])
        if moments is not None:
            m._m[n][:P].copy_(moments[0][n])
            m._v[n][:P].copy_(moments[1][n])
    m.P = P
    m._bind()
    m.fused_tail = True
    opt = G.GrowableAdam(m, **LRS)
    opt._step = step
    if voxels is not None:
        m.voxel_index.add(*voxels, 0)
    return m, opt


def _grads(m, seed):
    gen = torch.Generator().manual_seed(seed)
    P = m.P
    dev = m._xyz.device
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    return r(P, 3), [r(P, 3), r(P, 4), r(P, 1), r(P, m.M, 3)]


def _step(m, opt, g_xyz, g_act):
    m._xyz.grad = g_xyz.clone()
    m._act_grads = [g.clone() for g in g_act]
    opt.step_model(m)


def _state(m):
    return {n: (getattr(m, n).detach().clone(), m._m[n][:m.P].clone(), m._v[n][:m.P].clone()) for n in NAMES}


def _same_state(a, b):
    for n in NAMES:
        for x, y in zip(a[n], b[n]):
            assert x.shape == y.shape and torch.equal(x, y), n


def test_pruned_model_equals_a_model_rebuilt_from_the_kept_rows(gpu_device):
    dev, P, M = gpu_device, 2000, 4
    L = _leaves(P, M, dev, seed=8)
    rng = np.random.RandomState(0)
    vox_counts = []
    while sum(vox_counts) < P:
        vox_counts.append(min(int(rng.randint(0, 12)), P - sum(vox_counts)))
    vox_keys = (rng.permutation(50_000)[:len(vox_counts)] * 31 + 5).tolist()
    m, opt = _model(L, None, dev, voxels=(vox_keys, vox_counts))
    for it in range(3):                               # moments become non-zero
        _step(m, opt, *_grads(m, 20 + it))
    with torch.no_grad():                             # then about a third of the rows die, by rule and by mask
        dead = torch.rand(P, device=dev) < 0.3
        m._scaling[dead & (torch.arange(P, device=dev) % 2 == 0), 0] = 1.0
        m._opacity[dead & (torch.arange(P, device=dev) % 2 == 1)] = -8.0
    m._next_act = None
    mask = torch.rand(P, device=dev) < 0.05
    before = _state(m)
    out = m.prune(drop=mask)
    keep = out["reasons"] == 0
    assert torch.equal(keep, ~(dead | mask)) and out["P_after"] == int(keep.sum()) == m.P < P
    assert out["n_mask"] == int(mask.sum()) and out["n_opacity"] + out["n_scale"] >= int(dead.sum())
    assert torch.equal(out["row_map"], R.row_map_ref(out["reasons"]).cpu()) and opt._step == 3
    # the rebuilt model: t[keep] of every leaf and moment, the same step count, a fresh voxel index of the kept counts
    kept = {n: tuple(t[keep] for t in before[n]) for n in NAMES}
    first = np.cumsum([0] + vox_counts[:-1])
    k_np = keep.cpu().numpy()
    new_counts = [int(k_np[f:f + c].sum()) for f, c in zip(first, vox_counts)]
    ref, ref_opt = _model({n: kept[n][0] for n in NAMES}, ({n: kept[n][1] for n in NAMES}, {n: kept[n][2] for n in NAMES}),
                          dev, step=3, capacity=m.capacity, voxels=(vox_keys, new_counts))
    _same_state(_state(m), _state(ref))
    for k in vox_keys:
        assert m.voxel_index.get(k) == ref.voxel_index.get(k)
    for n in NAMES:                                   # the invariant add_new_pointcloud relies on
        assert not m._m[n][m.P:].any() and not m._v[n][m.P:].any() and m._m[n].shape[0] == m.capacity
        assert opt.state[getattr(m, n)]["exp_avg"].data_ptr() == m._m[n].data_ptr()
    # one further step on each: bit-identical parameters, moments and next activations
    g = _grads(m, 40)
    _step(m, opt, *g)
    _step(ref, ref_opt, *g)
    _same_state(_state(m), _state(ref))
    for x, y in zip(m._next_act, ref._next_act):
        assert torch.equal(x, y)
    # the similarity loss sees the same model: value and gradients
    gen = torch.Generator().manual_seed(2)
    picks = [vox_keys[i] for i in torch.randperm(len(vox_keys), generator=gen)[:30].tolist()]
    losses = {k: torch.randn((4, 3), generator=gen) for k in picks}
    vals = []
    for mod in (m, ref):
        mod.fused_tail = False
        loss = mod.calc_simi_loss(losses)
        loss.backward()
        vals.append((loss.detach(), mod._xyz.grad.clone(), mod._scaling.grad.clone()))
        mod._xyz.grad = mod._scaling.grad = None
        mod.fused_tail = True
    for x, y in zip(*vals):
        assert torch.equal(x, y)
    assert bool(vals[0][1].any())
    # growth after the prune lands at row P' with zero moments; a step then matches index_select + cat with zeros
    n_new = 70
    xyz = torch.randn((n_new, 3), device=dev)
    A = torch.randn((n_new, 3, 3), device=dev) * 0.05
    covs = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3, device=dev)
    rgbs = torch.rand((n_new, 3), device=dev) * 255
    P1 = m.P
    s_before = _state(m)
    assert m.add_new_pointcloud(xyz, covs, rgbs, 1.5, voxel_keys=[10 ** 9 + 1], voxel_counts=[n_new]) == (P1, P1 + n_new)
    assert m.voxel_index.get(10 ** 9 + 1) == (P1, n_new)
    s_after = _state(m)
    cat = {}
    for n in NAMES:
        assert torch.equal(s_after[n][0][:P1], s_before[n][0])
        assert not s_after[n][1][P1:].any() and not s_after[n][2][P1:].any()
        z = torch.zeros_like(s_after[n][0][P1:])
        cat[n] = (s_after[n][0].clone(), torch.cat([s_before[n][1], z]), torch.cat([s_before[n][2], z]))
    ref2, ref2_opt = _model({n: cat[n][0] for n in NAMES}, ({n: cat[n][1] for n in NAMES}, {n: cat[n][2] for n in NAMES}),
                            dev, step=4)
    g = _grads(m, 41)
    _step(m, opt, *g)
    _step(ref2, ref2_opt, *g)
    _same_state(_state(m), _state(ref2))
    with pytest.raises(KeyError):                     # a voxel the prune emptied is still registered
        m.add_new_pointcloud(xyz[:1], covs[:1], rgbs[:1], 1.5, voxel_keys=[vox_keys[0]], voxel_counts=[1])


def test_a_prune_that_drops_nothing_moves_nothing(gpu_device):
    dev = gpu_device
    m, opt = _model(_leaves(500, 4, dev, seed=1), None, dev)
    _step(m, opt, *_grads(m, 1))
    leaves = [getattr(m, n) for n in NAMES]
    act, bufs = m._next_act, [m._buf[n].data_ptr() for n in NAMES]
    assert act is not None
    out = m.prune()
    assert out["P_after"] == out["P_before"] == 500 and not out["reasons"].any()
    assert out["row_map"].tolist() == list(range(501))
    assert all(getattr(m, n) is p for n, p in zip(NAMES, leaves)) and m._next_act is act
    assert bufs == [m._buf[n].data_ptr() for n in NAMES] and opt._step == 1


@pytest.mark.parametrize("D", [0, 3])
@pytest.mark.parametrize("depth_gradient", [False, True])
def test_default_prune_changes_no_pixel_and_no_survivor_gradient(D, depth_gradient, gpu_device):
    dev, P, W, H = gpu_device, 2000, 160, 96
    sc, _ = R.prune_scene(P, W, H, 11, D)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    op = tt(sc["opacities"]).double()
    L = {"_xyz": tt(sc["means3D"]), "_features_dc": tt(sc["shs"][:, :1]), "_features_rest": tt(sc["shs"][:, 1:]),
         "_scaling": torch.log(tt(sc["scales"])), "_rotation": tt(sc["rotations"]) * 1.7,
         "_opacity": torch.log(op / (1 - op)).float()}
    m, _ = _model(L, None, dev)
    m.fused_tail = False
    settings = G.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], tt(sc["bg"]), 1.0, tt(sc["viewmatrix"]),
                                               tt(sc["projmatrix"]), D, tt(sc["campos"]), False, depth_gradient)
    gen = torch.Generator().manual_seed(6)
    wc, wa, wd = (torch.randn(s, generator=gen).to(dev) for s in ((3, H, W), (1, H, W), (1, H, W)))

    def render():
        xyz, opac, scales, rot, shs = m.activated()
        color, radii, depth, acc = G.GaussianRasterizer(settings)(xyz, torch.zeros_like(xyz), opac, shs=shs, scales=scales,
                                                                 rotations=rot)
        ((color * wc).sum() + (acc * wa).sum() + (depth * wd).sum()).backward()
        grads = [getattr(m, n).grad.clone() if getattr(m, n).grad is not None else None for n in NAMES]
        return color.detach(), depth.detach(), acc.detach(), radii, grads

    # one-chain frames, like the other modules' helper frames: these small renders must not feed the calling thread's
    # near/far history, which later tests' large frames start from
    prev = G.set_near_far_thread(False)
    try:
        c0, d0, a0, r0, g0 = render()
        out = m.prune()
        keep = out["reasons"] == 0
        c1, d1, a1, r1, g1 = render()
    finally:
        G.set_near_far_thread(prev)
    assert out["n_scale"] > 0 and 0.03 * P < out["n_opacity"] < 0.08 * P and out["n_nonfinite"] == 0 and m.P < P
    assert bool((r0[~keep & (out["reasons"] & R.SCALE).ne(0)] == 0).all())     # the scale-culled rows had no footprint
    assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(a0, a1)
    assert torch.equal(r1, r0[keep])
    for n, x, y in zip(NAMES, g0, g1):
        if x is None or x.numel() == 0:
            assert y is None or y.numel() == 0
            continue
        assert torch.equal(x[keep], y), n
        assert not x[~keep].any(), n          # the dropped rows were receiving no gradient: they were dead for good
    assert bool(g0[0].any()) and bool(g0[5].any())
