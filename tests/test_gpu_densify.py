"""GPU tests of adaptive density control (csrc/densify.hip through gsr_density_accumulate / gsr_densify_mark /
gsr_densify_apply, GrowableGaussians.densify).  The discrete outputs -- kinds, offsets, counts, every copied field, every
zero -- are compared exactly with tests/densify_ref.py; the continuous ones (the gradient sums, xyz and scaling of split
children) against its float64 evaluation at the bars its docstring counts.  The inputs are those of densify_cases.py,
on which test_densify_ref.py holds the float32 restatement to the same bars without a device."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi
from gs_livm_amd import synthetic as S

import densify_cases as Cs
import densify_ref as D
from arena import PAT, Arena, offsets

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
LRS = dict(position_lr=0.0005, feature_lr=0.001, opacity_lr=0.025, scaling_lr=0.0025, rotation_lr=0.0025)
SEED = 0xC0FFEE1234567


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- accumulate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", Cs.ACC_SIZES)
def test_accumulate_three_views(P, gpu_device):
    views, stats0, touched = Cs.accumulate_case(P)
    A = Arena(gpu_device, offsets("mix"))
    stats = A.put("stats", torch.from_numpy(stats0))
    s32, s64 = stats0.copy(), np.where(touched[:, None], np.zeros((P, 3)), np.nan)
    for v, (radii, g) in enumerate(views):
        r = torch.from_numpy(radii).to(gpu_device)
        grad = A.put("grad%d" % v, torch.from_numpy(g))
        _capi.density_accumulate(r, grad, stats)
        s32, s64 = D.accumulate(s32, radii, g, np.float32), D.accumulate(s64, radii, g, np.float64)
    got = stats.cpu().numpy()
    assert A.guards_intact() is None
    assert np.array_equal(got.view(np.uint32)[~touched], stats0.view(np.uint32)[~touched])   # untouched: bit for bit
    t = touched
    assert np.array_equal(got[t, 1:], s64[t, 1:])                                          # views and max_radius
    e_ref = np.abs(s32[t, 0].astype(np.float64) - s64[t, 0])
    bar = np.maximum(2 * e_ref, D.K_SUM * D.ULP * s64[t, 0])
    err = np.abs(got[t, 0].astype(np.float64) - s64[t, 0])
    ratio = float((err / np.maximum(bar, 1e-300)).max(initial=0))
    print("accumulate P=%d: worst error / bar %.3f" % (P, ratio))
    assert (err <= bar).all()


# ---- mark ------------------------------------------------------------------------------------------------------------
def _check_mark(stats, scaling, dev, grad_threshold, size_threshold, max_new):
    st, sc = torch.from_numpy(stats).to(dev), torch.from_numpy(scaling).to(dev)
    kinds, offs, counts = _capi.densify_mark(st, sc, grad_threshold, size_threshold, None if max_new < 0 else max_new)
    k, o, c = D.mark(stats, scaling, grad_threshold, size_threshold, max_new)
    assert np.array_equal(kinds.cpu().numpy(), k), max_new
    assert np.array_equal(offs.cpu().numpy(), o), max_new
    assert counts.tolist() == c, max_new
    return c


@pytest.mark.parametrize("P", Cs.MARK_SIZES)
def test_mark_is_the_float32_restatement(P, gpu_device):
    big = P > 100_000
    for pattern in (("0.05", "one_per_workgroup") if big else Cs.MARK_PATTERNS):
        stats, scaling, cand = Cs.mark_case(P, pattern)
        assert D.size_margin(scaling, Cs.SIZE_THRESHOLD) > 1e-5
        total = _check_mark(stats, scaling, gpu_device, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD, -1)[0]
        assert total == int(cand.sum())
        caps = {0, 1, total - 1, total, total + 1} | ({total // 2, int(cand[:1024 * 256].sum()) + 1} if big else set())
        for max_new in sorted(m for m in caps if m >= 0):
            _check_mark(stats, scaling, gpu_device, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD, max_new)


def test_mark_boundaries_and_empty_model(gpu_device):
    stats, scaling, want = Cs.mark_boundary_case()
    for max_new in (-1, 3, 100):
        c = _check_mark(stats, scaling, gpu_device, Cs.GRAD_THRESHOLD, 1.0, max_new)
    assert c == [int((want != 0).sum()), int((want == 1).sum()), int((want == 2).sum())]
    # a NaN threshold marks nothing
    assert _check_mark(stats, scaling, gpu_device, float("nan"), 1.0, -1) == [0, 0, 0]
    # P == 0: a no-op that yields n_new = 0
    e = torch.zeros((0, 3), device=gpu_device)
    kinds, offs, counts = _capi.densify_mark(e, e, 1.0, 1.0)
    assert kinds.numel() == 0 and offs.tolist() == [0] and counts.tolist() == [0, 0, 0]


# ---- apply -----------------------------------------------------------------------------------------------------------
def _arena_apply(P, M, dev, mode, leaves, moments, stats, kinds, offs, with_moments=True, with_stats=True, tail=5):
    """capacity buffers of P + n_new + tail rows at the arena's offsets: rows [P, ...) hold the NaN pattern"""
    n_new = int(offs[-1])
    cap = P + n_new + tail
    A = Arena(dev, offsets(mode))

    def grown(name, a):
        t = A.put(name, shape=(cap,) + a.shape[1:])
        _bits(t).fill_(PAT)
        t[:P].copy_(torch.from_numpy(a))
        return t
    p = [grown("p." + n, a) for n, a in zip(NAMES, leaves)]
    m = [grown("m." + n, a) for n, a in zip(NAMES, moments[:6])] if with_moments else None
    v = [grown("v." + n, a) for n, a in zip(NAMES, moments[6:])] if with_moments else None
    st = grown("stats", stats) if with_stats else None
    k = torch.from_numpy(kinds).to(dev)
    o = A.put("offsets", shape=(P + 1,)).view(torch.int32)
    o.copy_(torch.from_numpy(offs))
    return A, p, m, v, st, k, o, n_new


def _check_apply(P, M, dev, mode, seed=SEED, with_moments=True, with_stats=True):
    leaves, moments, stats, kinds, offs = Cs.apply_case(P, M)
    A, p, m, v, st, k, o, n_new = _arena_apply(P, M, dev, mode, leaves, moments, stats, kinds, offs, with_moments,
                                               with_stats)
    _capi.densify_apply(P, n_new, k, o, seed, p, m, v, st)
    torch.cuda.synchronize()
    assert A.guards_intact() is None
    out64, mom, st_ref = D.apply(leaves, kinds, offs, seed, np.float64, moments, stats)
    out32, _, _ = D.apply(leaves, kinds, offs, seed, np.float32)
    got = [t.cpu().numpy() for t in p]
    N = P + n_new
    for t in p + (m or []) + (v or []) + ([st] if st is not None else []):     # no row >= P + n_new is written
        assert bool((_bits(t[N:]) == PAT).all())
    sp, none = np.nonzero(kinds == 2)[0], np.nonzero(kinds == 0)[0]
    dsp = P + offs[sp]
    for idx in (1, 2, 4, 5):                                                   # copied fields, clones, kind 0: bit for bit
        assert np.array_equal(got[idx][:N].view(np.uint32), out32[idx].view(np.uint32)), NAMES[idx]
    rest = np.setdiff1d(np.arange(N), np.concatenate([sp, dsp]))
    for idx in (0, 3):
        assert np.array_equal(got[idx][rest].view(np.uint32), out32[idx][rest].view(np.uint32)), NAMES[idx]
    if with_moments:
        for t, ref in zip(m + v, mom):                                         # zeros written, clone parents kept
            assert np.array_equal(t[:N].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    if with_stats:
        assert np.array_equal(st[:N].cpu().numpy().view(np.uint32), st_ref.view(np.uint32))
    # the split children against float64 at the counted bars
    c64 = D.split_children(leaves[0], leaves[3], leaves[4], sp, seed, np.float64)
    worst = {"xyz": 0.0, "scaling": 0.0}
    for rows, truth in ((sp, c64[0]), (dsp, c64[1])):
        e_xyz = np.abs(out32[0][rows].astype(np.float64) - truth)
        bar = D.xyz_bar(e_xyz, c64[3], leaves[0][sp])
        err = np.abs(got[0][rows].astype(np.float64) - truth)
        worst["xyz"] = max(worst["xyz"], float((err / bar).max(initial=0)))
        assert (err <= bar).all()
        e_s = np.abs(out32[3][rows].astype(np.float64) - c64[2])
        bar = D.scale_bar(e_s, leaves[3][sp])
        err = np.abs(got[3][rows].astype(np.float64) - c64[2])
        worst["scaling"] = max(worst["scaling"], float((err / bar).max(initial=0)))
        assert (err <= bar).all()
    print("apply P=%d M=%d %s: worst error / bar %s" % (P, M, mode, {a: round(b, 3) for a, b in worst.items()}))
    return got, kinds, offs


@pytest.mark.parametrize("P,M", Cs.APPLY_CASES)
@pytest.mark.parametrize("mode", ("a0", "a4", "mix"))
def test_apply_clone_and_split(P, M, mode, gpu_device):
    _check_apply(P, M, gpu_device, mode)


def test_apply_without_moments_and_without_stats(gpu_device):
    _check_apply(300, 4, gpu_device, "a8", with_moments=False)
    _check_apply(300, 4, gpu_device, "a12", with_stats=False)
    _check_apply(257, 1, gpu_device, "mix", with_moments=False, with_stats=False)


def test_apply_is_reproducible_and_rows_are_independent(gpu_device):
    dev, P, M = gpu_device, 700, 4
    a, kinds, offs = _check_apply(P, M, dev, "a0")
    b, _, _ = _check_apply(P, M, dev, "a4")
    for x, y in zip(a, b):                                                     # same seed twice: identical bits
        n = P + int(offs[-1])
        assert np.array_equal(x[:n].view(np.uint32), y[:n].view(np.uint32))
    c, _, _ = _check_apply(P, M, dev, "a0", seed=SEED + 1)                      # another seed moves the split children only
    sp = np.nonzero(kinds == 2)[0]
    assert (a[0][sp] != c[0][sp]).any(1).mean() > 0.99
    cl = P + offs[np.nonzero(kinds == 1)[0]]
    assert np.array_equal(a[0][cl].view(np.uint32), c[0][cl].view(np.uint32))
    # another marked set: every second marked row loses its mark; the children of the rows still marked are unchanged,
    # although child 1 now lies in another row
    leaves, moments, stats, kinds, offs = Cs.apply_case(P, M)
    marked = np.nonzero(kinds)[0]
    kinds2 = kinds.copy()
    kinds2[marked[1::2]] = 0
    offs2 = np.concatenate([[0], np.cumsum(kinds2 != 0)]).astype(np.int32)
    A, p, m, v, st, k, o, n2 = _arena_apply(P, M, dev, "a0", leaves, moments, stats, kinds2, offs2)
    _capi.densify_apply(P, n2, k, o, SEED, p, m, v, st)
    d = [t.cpu().numpy() for t in p]
    assert A.guards_intact() is None
    still = np.nonzero(kinds2)[0]
    assert (offs2[still] != offs[still]).any()
    for x, y in zip(a, d):
        assert np.array_equal(x[still].view(np.uint32), y[still].view(np.uint32))
        assert np.array_equal(x[P + offs[still]].view(np.uint32), y[P + offs2[still]].view(np.uint32))


# ---- the model -------------------------------------------------------------------------------------------------------
def _model(sc, dev, capacity=None):
    """a GrowableGaussians holding the scene's Gaussians as raw leaves, its capacity exactly P, with a GrowableAdam"""
    P, M = sc["means3D"].shape[0], sc["shs"].shape[1]
    m = G.GrowableGaussians(capacity or P, M, dev)
    with torch.no_grad():
        b = m._buf
        b["_xyz"][:P] = torch.from_numpy(sc["means3D"])
        b["_features_dc"][:P] = torch.from_numpy(sc["shs"][:, :1])
        b["_features_rest"][:P] = torch.from_numpy(sc["shs"][:, 1:])
        b["_scaling"][:P] = torch.from_numpy(np.log(sc["scales"]))
        b["_rotation"][:P] = torch.from_numpy(sc["rotations"])
        o = sc["opacities"].astype(np.float64)
        b["_opacity"][:P] = torch.from_numpy(np.log(o / (1 - o)).astype(np.float32))
    m.P = P
    m.voxel_index.add([11, 22, 33], [P // 3, P // 3, P - 2 * (P // 3)], 0)
    m._bind()
    return m, G.GrowableAdam(m, **LRS)


def _one_step(m, opt, gen):
    m.fused_tail = True
    xyz, opac, scales, rot, shs = m.activated()
    w = [torch.randn(t.shape, generator=gen).to(t.device) for t in (xyz, opac, scales, rot, shs)]
    sum((t * x).sum() for t, x in zip((xyz, opac, scales, rot, shs), w)).backward()
    opt.step_model(m)


def test_model_densify_reserves_steps_and_keeps_its_books(gpu_device):
    from helpers import hip_backward, hip_forward
    dev = gpu_device
    sc = S.make_scene(300, 70, 50, 11, sh_degree=1)
    m, opt = _model(sc, dev)
    P = m.P
    assert m.capacity == P
    gen = torch.Generator().manual_seed(1)
    _one_step(m, opt, gen)                                    # non-zero moments everywhere
    m.enable_density_stats()
    t, fwd = hip_forward(sc, dev, debug=False)                # (only the statistics' inputs are taken from this frame)
    dcol, dacc = S.make_upstream_grads(sc["W"], sc["H"], 11)
    g2d = torch.from_numpy(hip_backward(sc, t, fwd, dcol, dacc, dev, debug=False)["dL_dmeans2D"]).to(dev)
    radii = fwd[4]
    for _ in range(2):
        m.accumulate_density(radii, g2d)
    st = m.density_stats().cpu().numpy()
    vis = radii.cpu().numpy() > 0
    assert vis.any() and (st[vis, 1] == 2).all() and not st[~vis].any()
    avg = st[vis, 0] / st[vis, 1]
    thr = float(np.median(avg))
    size = float(np.median(np.exp(m._scaling.detach().cpu().numpy()).max(1)))
    before = {n: getattr(m, n).detach().clone() for n in NAMES}
    mom_before = {n: [x.clone() for x in m.moments(n)] for n in NAMES}
    vox_before = dict(m.voxel_index._ranges)
    ref_k, ref_o, ref_c = D.mark(st, before["_scaling"].cpu().numpy(), thr, size)
    assert D.size_margin(before["_scaling"].cpu().numpy()[ref_k != 0], size) > 1e-5
    out = m.densify(thr, size, seed=5)
    n_new = out["n_new"]
    assert [n_new, out["n_clone"], out["n_split"]] == ref_c and out["n_clone"] > 0 and out["n_split"] > 0
    assert np.array_equal(out["kinds"].cpu().numpy(), ref_k) and np.array_equal(out["offsets"].numpy(), ref_o)
    assert m.P == P + n_new == out["P_after"] and m.capacity >= m.P > P        # the capacity was P: it reserved
    assert m.voxel_index._ranges == vox_before                                 # appended rows belong to no voxel
    assert not m._stats.any()
    kinds, offs = torch.from_numpy(ref_k).to(dev), torch.from_numpy(ref_o[:-1].astype(np.int64)).to(dev)
    cl, sp, none = kinds == 1, kinds == 2, kinds == 0
    for n in NAMES:
        now, (ma, va) = getattr(m, n).detach(), m.moments(n)
        assert torch.equal(now[:P][none], before[n][none]) and torch.equal(now[P + offs[cl]], before[n][cl])
        for x, x0 in ((ma, mom_before[n][0]), (va, mom_before[n][1])):
            assert torch.equal(x[:P][~sp], x0[~sp])                            # clone parents and kind 0 keep their moments
            assert not x[:P][sp].any() and not x[P:].any()                     # split parents and new rows start fresh
        assert not m._m[n][m.P:].any() and not m._v[n][m.P:].any()
    assert opt.state[m._xyz]["exp_avg"].data_ptr() == m._m["_xyz"].data_ptr()
    step = opt._step
    _one_step(m, opt, gen)                                                     # step_model runs on the densified model
    assert opt._step == step + 1 and bool(torch.isfinite(m._xyz).all()) and m._m["_xyz"][P:m.P].any()
    # a prune afterwards carries the statistics with their rows
    m._stats[:m.P] = torch.arange(m.P, device=dev, dtype=torch.float32)[:, None].expand(-1, 3)
    drop = torch.zeros(m.P, dtype=torch.bool, device=dev)
    drop[::3] = True
    pr = m.prune(min_opacity=0.0, max_scale=float("inf"), drop=drop)
    keep = (~drop).nonzero().reshape(-1).float()
    assert pr["P_after"] == keep.numel() == m.P
    assert torch.equal(m.density_stats(), keep[:, None].expand(-1, 3)) and not m._stats[m.P:].any()
    # add_new_pointcloud lands behind the new rows with zero moments
    n = 40
    lo, hi = m.add_new_pointcloud(torch.randn(n, 3, device=dev), torch.eye(3, device=dev).repeat(n, 1, 1) * 0.01,
                                  torch.rand(n, 3, device=dev) * 255, voxel_keys=[44], voxel_counts=[n])
    assert (lo, hi) == (pr["P_after"], pr["P_after"] + n) and m.voxel_index.get(44) == (lo, n)
    for name in NAMES:
        assert not m._m[name][lo:hi].any() and not m._v[name][lo:hi].any()
    assert not m._stats[lo:hi].any()


def test_model_without_candidates_keeps_its_leaf_objects(gpu_device):
    sc = S.make_scene(100, 64, 48, 3, sh_degree=0)
    m, opt = _model(sc, gpu_device)
    with pytest.raises(RuntimeError):
        m.densify(1.0, 1.0)                                                    # the statistics were never enabled
    m.enable_density_stats()
    m.fused_tail = True
    m.activated()
    m._next_act = cached = ("kept",)
    leaves = [getattr(m, n) for n in NAMES]
    out = m.densify(1.0, 1.0)
    assert out["n_new"] == 0 and out["P_after"] == 100 and not out["kinds"].any()
    assert all(getattr(m, n) is leaf for n, leaf in zip(NAMES, leaves)) and m._next_act is cached
    m._next_act = None


def test_densified_model_is_a_legal_model(gpu_device):
    """forward and backward of the densified model at a small frame against the oracle and the f64 restatement, with the
    suite's own helpers and bars (helpers.check_against_ref64)"""
    import ref64 as R64
    from helpers import GRAD_NAMES, check_against_ref64, hip_backward, hip_forward, masked_upstream
    from oracle import oracle as O
    dev, seed = gpu_device, 11
    sc = S.make_scene(300, 70, 50, seed, sh_degree=3)
    m, _ = _model(sc, dev)
    m.enable_density_stats()
    m._stats[:m.P, 0] = torch.rand(m.P, device=dev)
    m._stats[:m.P, 1] = 1.0
    out = m.densify(0.5, 0.045, seed=9)
    assert out["n_clone"] > 20 and out["n_split"] > 20
    with torch.no_grad():
        xyz, opac, scales, rot, shs = m.activated()
    sc2 = dict(sc)
    sc2.update(means3D=xyz.detach().cpu().numpy(), opacities=opac.cpu().numpy(), scales=scales.cpu().numpy(),
               rotations=rot.cpu().numpy(), shs=shs.cpu().numpy())
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc2)
    dcol, dacc = masked_upstream(sc2["W"], sc2["H"], seed, fr.fragile)
    r = R64.render(sc2, fr, dcol, dacc, slack=True)
    t, fwd = hip_forward(sc2, dev, debug=False)
    assert np.array_equal(fwd[4].cpu().numpy(), fr.radii)
    got = hip_backward(sc2, t, fwd, dcol, dacc, dev, debug=False)
    images = {"out_color": fwd[1].cpu().numpy(), "out_depth": fwd[2].cpu().numpy(), "out_acc": fwd[3].cpu().numpy()}
    check_against_ref64(r, fr.fragile, images, {k: got[k] for k in GRAD_NAMES})


def test_render_full_hands_out_radii_and_the_means2D_leaf(gpu_device):
    from gs_livm_amd.render_utils import Camera, render, render_full
    dev = gpu_device
    sc = S.make_scene(200, 64, 48, 5, sh_degree=0)
    m, _ = _model(sc, dev)
    m.enable_density_stats()
    cam = Camera(np.eye(3), np.zeros(3), 2 * np.arctan(sc["tanfovx"]), 2 * np.arctan(sc["tanfovy"]), 64, 48, device=dev)
    bg = torch.ones(3, device=dev)
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        color, depth, acc, radii, means2D = render_full(cam, m, bg)
        plain = render(cam, m, bg)
    finally:
        G.set_near_far_thread(prev_nf)
    assert torch.equal(color, plain[0]) and torch.equal(depth, plain[1]) and torch.equal(acc, plain[2])
    assert radii.dtype == torch.int32 and radii.shape == (200,) and means2D.shape == (200, 3) and means2D.is_leaf
    color.square().sum().backward()
    assert means2D.grad is not None and bool((means2D.grad[radii > 0] != 0).any())
    m.accumulate_density(radii, means2D.grad)
    st = m.density_stats()
    assert torch.equal(st[:, 1], (radii > 0).float())
    assert torch.allclose(st[:, 0][radii > 0], means2D.grad[radii > 0][:, :2].norm(dim=1), rtol=1e-6, atol=0)
