"""GPU tests of the sweep voxel map (csrc/voxel.hip: gsr_voxel_sweep, gsr_voxel_rehash; voxelmap.py, model.py
add_voxel_seeds, torch_next.cpp) against its float64 restatement (tests/voxel_ref.py), whose docstring derives the bars.

Exact: the table's state, the statuses, the point keys, the six counts and the order of the seeds, bit for bit, on
every case of voxel_ref; a permuted sweep, two runs, sessions over three sweeps, the compaction across workgroup seams,
grow / rehash, a full table, guarded buffers at 0/4/8/12 bytes (the int64 arrays at 0/8: they need 8-byte alignment and
are refused elsewhere), refusals that write nothing, the C++ route.  Against float64: xyz and rgbs within one f32 ulp of
the narrowed restatement, covs and the covariance rebuilt from (scaling_raw, rotation) at COV_BAR / RECON_BAR, the
normal at NORMAL_BAR.  Every float comparison prints its worst |error| / bar; DESIGN.md section 2, "Sweep voxel map",
records them."""
import ctypes as C

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import ref64
import voxel_ref as vr
from arena import PAT, Arena, offsets

pytestmark = pytest.mark.gpu
I64 = ("table", "point_keys", "keys")
F32_OUT = dict(xyz=3, covs=9, rgb=3, npoints=1, scaling=3, rotation=4, normal=3)   # (npoints: the int32 counts)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _state_equal(got, want):
    for k in want:
        g = _np(got[k]) if isinstance(got[k], torch.Tensor) else got[k]
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), k


def _exact_part(seeds, ref):
    """status, point keys, counts, the seeds' keys (in order) and point counts."""
    assert np.array_equal(_np(seeds.status), ref["status"])
    assert np.array_equal(_np(seeds.point_keys), ref["point_keys"])
    assert tuple(seeds.counts) == tuple(ref["counts"])
    assert _np(seeds.keys).tolist() == [s.key for s in ref["seeds"]]
    assert _np(seeds.points).tolist() == [s.count for s in ref["seeds"]]


def _float_part(seeds, ref, scale_factor=1.0, what=""):
    """The continuous outputs of every seed against float64; returns the worst ratios."""
    rs = ref["seeds"]
    v = len(rs)
    if v == 0:
        return {}
    xyz, covs, rot, raw = _np(seeds.xyz), _np(seeds.covs).astype(np.float64), _np(seeds.rotation), _np(seeds.scaling_raw)
    d = vr.ulp_distance(xyz, np.stack([s.xyz32 for s in rs]))
    out = dict(xyz_ulp=int(d.max()), xyz_share=float((d > 0).mean()))
    if seeds.rgbs is not None:
        d = vr.ulp_distance(_np(seeds.rgbs), np.stack([s.rgb32 for s in rs]))
        out.update(rgb_ulp=int(d.max()), rgb_share=float((d > 0).mean()))
    assert np.array_equal(covs, covs.transpose(0, 2, 1))
    qn = np.linalg.norm(rot.astype(np.float64), axis=1)
    assert (rot[:, 0] >= 0).all() and np.abs(qn - 1.0).max() <= 4 * vr.U
    # Sigma as the rasterizer builds it from the activated scales and the quaternion as stored
    c6 = ref64.cov3d(torch.from_numpy(np.exp(raw.astype(np.float64))), torch.from_numpy(rot.astype(np.float64)), 1.0,
                     departures=False).numpy()
    ix = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov_r = recon_r = 0.0
    for j, s in enumerate(rs):
        lam_max = float(s.lam[0])
        L = float(np.abs(s.scaling_raw).max())
        want = s.cov * float(np.float32(scale_factor))
        cov_r = max(cov_r, np.abs(covs[j] - s.cov).max() / vr.cov_bar(lam_max))
        got = np.array([c6[j][k] for k in range(6)])
        recon_r = max(recon_r, max(abs(got[k] - want[a][b]) for k, (a, b) in enumerate(ix)) /
                      vr.recon_bar(lam_max, L, float(np.float32(scale_factor))))
    out.update(cov_ratio=cov_r, recon_ratio=recon_r)
    print("voxel %s: %s" % (what, out))
    assert out["xyz_ulp"] <= vr.XYZ_ULPS and out.get("rgb_ulp", 0) <= vr.XYZ_ULPS
    assert cov_r <= 1.0 and recon_r <= 1.0
    return out


def _run(dev, grid, cases, min_points=4, min_sigma=0.001, colours=True, capacity=64):
    """The sweeps of `cases` into one device map and one reference map; returns both and the last results."""
    m, r = G.SweepVoxelMap(grid, min_points, min_sigma, capacity=capacity, device=dev), vr.RefMap(grid, min_points, min_sigma)
    for pts, cols in cases:
        s = m.sweep(_t(pts, dev), _t(cols, dev) if colours else None)
        w = r.sweep(pts, cols if colours else None)
        _exact_part(s, w)
        _state_equal(m.state(), r.state())
        assert (s.rgbs is None) == (not colours)
        _float_part(s, w, what="grid %s n %d" % (grid, len(pts)))
    return m, r


@pytest.mark.parametrize("colours", (True, False))
@pytest.mark.parametrize("grid", vr.GRIDS)
def test_state_statuses_and_counts_bit_for_bit(gpu_device, grid, colours):
    # every size into ONE map: later sweeps meet voxels that earlier ones opened or closed
    _run(gpu_device, grid, [vr.random_cloud(n) for n in vr.SIZES], colours=colours)
    _run(gpu_device, grid, [vr.one_voxel(grid=grid)], colours=colours)            # 1 025 threads on one slot
    _run(gpu_device, grid, [vr.distinct_voxels(grid=grid)], min_points=1, colours=colours)
    _run(gpu_device, grid, [vr.boundary_points(grid)], min_points=1, colours=colours)


def test_a_permuted_sweep_and_a_second_run_give_the_same_bits(gpu_device):
    dev = gpu_device
    pts, cols = vr.random_cloud(1025)
    perm = np.random.RandomState(5).permutation(len(pts))
    for grid in vr.GRIDS:
        runs = []
        for p, c in ((pts, cols), (pts, cols), (pts[perm], cols[perm])):
            m = G.SweepVoxelMap(grid, 4, 0.001, capacity=4096, device=dev)
            runs.append((m.state(), m.sweep(_t(p, dev), _t(c, dev)), m.state()))
        a, b, c = runs
        for f in G.VoxelSeeds._fields:
            if f != "counts":
                assert torch.equal(getattr(a[1], f), getattr(b[1], f)), f      # two runs: the same bits, order included
        assert a[1].counts == b[1].counts == c[1].counts and a[1].counts[4] > 100
        _state_equal(a[2], {k: _np(v) for k, v in b[2].items()})
        _state_equal(a[2], {k: _np(v) for k, v in c[2].items()})
        # the permuted sweep: the same seeds as a set keyed by key
        ka, kc = _np(a[1].keys), _np(c[1].keys)
        assert ka.tolist() != kc.tolist() and sorted(ka.tolist()) == sorted(kc.tolist())
        oa, oc = np.argsort(ka), np.argsort(kc)
        for f in ("xyz", "covs", "rgbs", "points", "scaling_raw", "rotation", "normal"):
            assert np.array_equal(_np(getattr(a[1], f))[oa].view(np.int32), _np(getattr(c[1], f))[oc].view(np.int32)), f
        pd = torch.from_numpy(perm).to(dev)
        assert torch.equal(a[1].status[pd], c[1].status) and torch.equal(a[1].point_keys[pd], c[1].point_keys)


def test_sessions_a_voxel_matures_over_two_sweeps_and_then_takes_no_more(gpu_device):
    dev = gpu_device
    pts, cols = vr.one_voxel(n=12)
    far = vr.distinct_voxels(n=5)
    m, r = G.SweepVoxelMap(0.25, 10, 0.001, capacity=64, device=dev), vr.RefMap(0.25, 10, 0.001)
    for k, (p, c) in enumerate(((pts[:6], cols[:6]), (np.concatenate([far[0], pts[6:]]), np.concatenate([far[1], cols[6:]])),
                                (pts, cols))):
        s, w = m.sweep(_t(p, dev), _t(c, dev)), r.sweep(p, c)
        before = m.state()
        _exact_part(s, w)
        _state_equal(before, r.state())
        _float_part(s, w, what="session %d" % k)
        if k == 0:
            assert s.counts == (6, 0, 0, 0, 0, 1)
        if k == 1:
            assert s.counts == (11, 0, 0, 0, 1, 6) and int(s.points[0]) == 12
    assert s.counts == (0, 12, 0, 0, 0, 6) and bool((s.status == vr.SEEDED).all())
    again = m.sweep(_t(pts, dev), _t(cols, dev))                              # SEEDED points move nothing
    _state_equal(m.state(), {k: _np(v) for k, v in before.items()})
    assert again.counts == s.counts


@pytest.mark.parametrize("pattern", ("all", "none", "every_other", "every_third"))
def test_the_seed_order_is_first_appearance_across_workgroup_seams(gpu_device, pattern):
    dev = gpu_device
    nv = 600                                                                     # owners in three workgroups
    first, cols = vr.distinct_voxels(n=nv)
    pick = dict(all=np.ones(nv, bool), none=np.zeros(nv, bool), every_other=np.arange(nv) % 2 == 0,
                every_third=np.arange(nv) % 3 == 1)[pattern]
    order = np.random.RandomState(2).permutation(nv)                             # first appearance != key order
    second = order[pick[order]][::-1]                                            # the second points come in another order
    pts = np.concatenate([first[order], first[second]])
    cl = np.concatenate([cols[order], cols[second]])
    m, r = G.SweepVoxelMap(0.25, 2, 0.001, capacity=4096, device=dev), vr.RefMap(0.25, 2, 0.001)
    s, w = m.sweep(_t(pts, dev), _t(cl, dev)), r.sweep(pts, cl)
    _exact_part(s, w)
    _state_equal(m.state(), r.state())
    want = vr.cells(first[order][pick[order]], 0.25)[3]
    assert _np(s.keys).tolist() == want.tolist() and s.counts[4] == int(pick.sum())
    if pattern == "all":
        assert _np(s.keys).tolist() != sorted(_np(s.keys).tolist())              # not the order of the keys


@pytest.mark.parametrize("grid", vr.GRIDS)
def test_plane_scenes_against_float64(gpu_device, grid):
    dev = gpu_device
    worst = 0.0
    for which in range(len(vr.PLANES)):
        pts, cols, nrm = vr.plane_scene(which)
        m = G.SweepVoxelMap(grid, vr.PLANE_MIN_POINTS, vr.PLANE_MIN_SIGMA, capacity=8192, device=dev)
        r = vr.RefMap(grid, vr.PLANE_MIN_POINTS, vr.PLANE_MIN_SIGMA)
        s, w = m.sweep(_t(pts, dev), _t(cols, dev), scale_factor=1.5), r.sweep(pts, cols, scale_factor=1.5)
        _exact_part(s, w)
        _float_part(s, w, scale_factor=1.5, what="plane %d grid %s" % (which, grid))
        normal = _np(s.normal).astype(np.float64)
        for j, sd in enumerate(w["seeds"]):
            sign = 1.0 if float(normal[j] @ sd.normal) >= 0 else -1.0
            bar = vr.normal_bar(float(sd.lam_raw[0]), float(sd.lam_raw[1] - sd.lam_raw[2]))
            worst = max(worst, np.abs(sign * normal[j] - sd.normal).max() / bar)
        # every matured voxel is a flat surfel along the plane: the last scale is the smallest by a wide margin
        raw = _np(s.scaling_raw)
        assert (raw[:, 0] >= raw[:, 1]).all() and (raw[:, 1] > raw[:, 2] + 1.0).all()
        assert np.abs(normal @ nrm).min() >= 0.988
    print("voxel normals grid %s: worst |error| / bar %.3f" % (grid, worst))
    assert worst <= 1.0


def test_the_min_sigma_clamp_on_a_collinear_and_a_single_point_voxel(gpu_device):
    dev = gpu_device
    for pts, cols, mp, ms in (vr.collinear_voxel(0.25) + (10, 0.001),
                              (np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[10.0, 20.0, 30.0]], np.float32), 1, 0.002)):
        m, r = G.SweepVoxelMap(0.25, mp, ms, capacity=64, device=dev), vr.RefMap(0.25, mp, ms)
        s, w = m.sweep(_t(pts, dev), _t(cols, dev)), r.sweep(pts, cols)
        _exact_part(s, w)
        _float_part(s, w, what="clamp n %d" % len(pts))
        floor = np.float32(np.log(np.sqrt(float(np.float32(ms)) ** 2)))
        raw = _np(s.scaling_raw)[0]
        assert raw[2] == floor and raw[1] == floor and (len(pts) == 1) == (raw[0] == floor)


def test_grow_and_rehash_keep_the_state(gpu_device):
    dev = gpu_device
    pts, cols = vr.random_cloud(1025)
    m = G.SweepVoxelMap(0.2, 4, 0.001, capacity=4096, device=dev)
    m.sweep(_t(pts, dev), _t(cols, dev))
    before, live = m.state(), m.live
    old = m.table.clone()
    m.grow()
    assert m.capacity == 8192 and m.live == live
    _state_equal(m.state(), {k: _np(v) for k, v in before.items()})
    m.grow(1 << 15)
    _state_equal(m.state(), {k: _np(v) for k, v in before.items()})
    same = G._capi.voxel_rehash(old, G._capi.voxel_table(4096, dev))             # the same capacity is legal
    assert int((same[:, 0] != 0).sum()) == live == before["keys"].numel()
    # a small table that had to grow inside sweep() holds what a large one holds, and sees the same later sweeps
    small = G.SweepVoxelMap(0.2, 4, 0.001, capacity=2, device=dev)
    small.sweep(_t(pts, dev), _t(cols, dev))
    assert small.capacity >= 2 * 1025
    _state_equal(small.state(), {k: _np(v) for k, v in before.items()})
    a, b = m.sweep(_t(pts[:300], dev), _t(cols[:300], dev)), small.sweep(_t(pts[:300], dev), _t(cols[:300], dev))
    assert a.counts == b.counts and torch.equal(a.status, b.status) and a.counts[1] > 0 and a.counts[3] == 0


def _raw(dev, pts, cols, mode="a0", grid=0.25, min_points=1, min_sigma=0.001, sf=1.0, capacity=64, live=0,
         shift=None, n=None):
    """gsr_voxel_sweep through ctypes with every tensor, the table and the workspace (exactly the queried size) inside
    guarded allocations prefilled with arena.PAT; the int64 arrays at the offset's multiple of 8.  shift: {name: bytes}
    to move single tensors.  Returns (arena, return code)."""
    lib = G.lib()
    n = len(pts) if n is None else n
    rows = max(len(pts), 1)
    base = offsets(mode)

    def off(name, i):
        o = base(name, i) & ~4 if name in I64 else base(name, i)
        return (shift or {}).get(name, o)

    ar = Arena(dev, off)
    ar.put("points", _t(np.asarray(pts, np.float32).reshape(-1, 3), dev))
    if cols is not None:
        ar.put("colors", _t(np.asarray(cols, np.float32).reshape(-1, 3), dev))
    ar.put("table", shape=(capacity * 32,)).view(torch.int32).zero_()
    ar.put("status", shape=((rows + 3) // 4 + 1,))
    ar.put("point_keys", shape=(2 * rows,))
    ar.put("keys", shape=(2 * rows,))
    for k, wd in F32_OUT.items():
        if k != "rgb" or cols is not None:
            ar.put(k, shape=(rows, wd))
    ar.put("counts", shape=(6,))
    nbytes = int(lib.gsr_voxel_sweep_workspace(n)) if 0 <= n <= 1 << 22 else 0
    assert nbytes % 4 == 0
    ar.put("ws", shape=(max(nbytes // 4, 1),))
    p = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t and ar.ptr(k) else None  # noqa: E731
    rc = lib.gsr_voxel_sweep(n, p("points"), p("colors"), grid, min_points, min_sigma, sf, p("table"), capacity, live,
                             p("status"), p("point_keys"), p("xyz"), p("covs"), p("rgb"), p("keys"), p("npoints"),
                             p("scaling"), p("rotation"), p("normal"), p("counts"), p("ws"), nbytes,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ar, rc


def _bits(ar, name, dtype=np.int32):
    return ar.t[name].view(torch.int32).cpu().numpy().reshape(-1).view(dtype)


def test_a_full_table_ends_and_counts_eight_and_eight(gpu_device):
    pts, cols = vr.distinct_voxels(n=16)
    ar, rc = _raw(gpu_device, pts, cols, capacity=8, min_points=5)
    assert rc == 0 and ar.guards_intact() is None
    status = _bits(ar, "status", np.uint8)[:16]
    assert int((status == vr.FULL).sum()) == 8 and int((status == vr.ACCUMULATED).sum()) == 8
    assert _bits(ar, "counts").tolist() == [8, 0, 0, 8, 0, 8]
    keys = _bits(ar, "point_keys", np.int64)[:16]
    assert np.array_equal(keys, vr.cells(pts, 0.25)[3])                         # a FULL point still has its key
    table = _bits(ar, "table", np.int64).reshape(8, 16)
    assert (table[:, 0] != 0).all() and set(table[:, 0].tolist()) == set(keys[status == vr.ACCUMULATED].tolist())
    assert (table[:, 2] == 1).all() and (table[:, 15] == 0).all() and (table[:, 1] == 0).all()


@pytest.mark.parametrize("mode", ("a0", "a4", "a8", "a12", "mix"))
def test_guarded_buffers_at_every_offset(gpu_device, mode):
    pts, cols = vr.random_cloud(257)
    ref = vr.RefMap(0.2, 3, 0.001)
    w = ref.sweep(pts, cols, scale_factor=2.0)
    v = w["counts"][4]
    assert 0 < v < 257
    ar, rc = _raw(gpu_device, pts, cols, mode=mode, grid=0.2, min_points=3, sf=2.0, capacity=1024)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None
    assert np.array_equal(_bits(ar, "status", np.uint8)[:257], w["status"])
    assert np.array_equal(_bits(ar, "status", np.uint8)[257:], np.full(66, PAT, np.int32).view(np.uint8)[257:])
    assert np.array_equal(_bits(ar, "point_keys", np.int64), w["point_keys"])
    assert _bits(ar, "counts").tolist() == list(w["counts"])
    assert _bits(ar, "keys", np.int64)[:v].tolist() == [s.key for s in w["seeds"]]
    assert (_bits(ar, "keys")[2 * v:] == PAT).all()
    for k, wd in F32_OUT.items():                                               # rows at and behind the seed count
        b = _bits(ar, k).reshape(-1, wd)
        assert (b[v:] == PAT).all() and not (b[:v] == PAT).any(), k
    assert vr.ulp_distance(_bits(ar, "xyz", np.float32).reshape(-1, 3)[:v],
                           np.stack([s.xyz32 for s in w["seeds"]])).max() <= vr.XYZ_ULPS
    table = _bits(ar, "table", np.int64).reshape(1024, 16)
    live = table[table[:, 0] != 0]
    live = live[np.argsort(live[:, 0])]
    st = ref.state()
    assert np.array_equal(live[:, 0], st["keys"]) and np.array_equal(live[:, 1], st["closed"])
    assert np.array_equal(live[:, 2], st["count"]) and np.array_equal(live[:, 6:12], st["s2"]) and (live[:, 15] == 0).all()


def test_refusals_write_nothing(gpu_device):
    dev = gpu_device
    pts, cols = vr.random_cloud(65)
    err = G.lib().gsr_last_error
    for kw, what in ((dict(grid=0.0), b"bad grid"), (dict(grid=float("nan")), b"bad grid"),
                     (dict(grid=float("inf")), b"bad grid"), (dict(min_sigma=-1.0), b"bad min_sigma"),
                     (dict(min_points=0), b"bad min_points"), (dict(min_points=(1 << 20) + 1), b"bad min_points"),
                     (dict(n=(1 << 22) + 1), b"bad n"), (dict(n=-1), b"bad n"), (dict(capacity=48), b"bad capacity"),
                     (dict(sf=0.0), b"bad scale_factor"), (dict(live=65), b"bad live_before"),
                     (dict(shift={"table": 4}), b"8-byte"), (dict(shift={"keys": 12}), b"8-byte"),
                     (dict(shift={"point_keys": 4}), b"8-byte")):
        ar, rc = _raw(dev, pts, cols, **kw)
        assert rc == -1 and what in err(), (kw, err())
        assert ar.guards_intact() is None
        for k in ("status", "point_keys", "keys", "counts", "ws") + tuple(F32_OUT):
            assert (_bits(ar, k) == PAT).all(), (kw, k)
        assert (_bits(ar, "table") == 0).all(), kw


def test_the_cpp_route_gives_the_python_routes_bits(gpu_device):
    dev = gpu_device
    nx = G.torch_ops().next
    pts, cols = vr.random_cloud(1025)
    m = G.SweepVoxelMap(0.2, 4, 0.001, capacity=64, device=dev)
    table, live = nx.voxel_table(64, _t(pts, dev)), 0
    for lo, hi, colours in ((0, 300, True), (300, 1025, True), (0, 1025, True)):
        p, c = _t(pts[lo:hi], dev), _t(cols[lo:hi], dev)
        a = m.sweep(p, c, scale_factor=1.25)
        b, table, live = nx.voxel_sweep(table, live, p, c, 0.2, 4, 0.001, 1.25)
        assert live == m.live and table.size(0) == m.capacity
        for f, y in zip(G.VoxelSeeds._fields, b):
            x = getattr(a, f)
            assert (x == tuple(y)) if f == "counts" else torch.equal(x, y), f
    st = m.state()
    t = table.cpu()
    t = t[t[:, 0] != 0]
    t = t[torch.argsort(t[:, 0])]
    assert torch.equal(t[:, 0], st["keys"]) and torch.equal(t[:, 2], st["count"]) and torch.equal(t[:, 6:12], st["s2"])
    assert a.counts[1] > 0 and a.counts[0] > 0
    none = nx.voxel_sweep(table, live, _t(pts[:10], dev), None, 0.2, 4, 0.001)[0]
    assert none[2] is None


def test_add_voxel_seeds_registers_the_voxels_and_feeds_the_similarity_loss(gpu_device):
    dev = gpu_device
    pts, cols, _ = vr.plane_scene(2)
    m = G.SweepVoxelMap(0.25, 10, 0.001, capacity=4096, device=dev)
    seeds = m.sweep(_t(pts, dev), _t(cols, dev))
    v = seeds.counts[4]
    model, plain = G.GrowableGaussians(16, 4, dev), G.GrowableGaussians(16, 4, dev)
    G.GrowableAdam(model)
    assert model.calc_simi_loss({}) is None
    assert model.add_voxel_seeds(seeds) == (0, v) and model.P == v
    keys = _np(seeds.keys).tolist()
    for j, k in enumerate(keys):
        assert model.voxel_index.get(k) == (j, 1)
    assert torch.equal(model._scaling.data, seeds.scaling_raw) and torch.equal(model._rotation.data, seeds.rotation)
    assert torch.equal(model._xyz.data, seeds.xyz)
    # oriented=False is add_new_pointcloud, bit for bit
    other = G.GrowableGaussians(16, 4, dev)
    assert other.add_voxel_seeds(seeds, oriented=False) == (0, v)
    assert plain.add_new_pointcloud(seeds.xyz, seeds.covs, seeds.rgbs, 1.0) == (0, v)
    for name in G.GrowableGaussians._NAMES:
        assert torch.equal(getattr(other, name).data, getattr(plain, name).data), name
        if name not in ("_scaling", "_rotation"):
            assert torch.equal(getattr(model, name).data, getattr(plain, name).data), name
    assert not torch.equal(model._rotation.data, plain._rotation.data)
    # a second sweep over the same surface: its points are SEEDED and select the rows of their voxels
    again = m.sweep(_t(pts, dev), _t(cols, dev))
    assert again.counts[1] > 500 and again.counts[4] >= 0
    losses = m.loss_points(_t(pts, dev), again, max_points=7)
    assert set(losses) <= set(keys) and len(losses) > 30
    assert all(t.shape[1] == 3 and 1 <= t.shape[0] <= 7 and t.dtype == torch.float32 for t in losses.values())
    k0 = next(iter(losses))
    mine = pts[(vr.cells(pts, 0.25)[3] == k0) & (_np(again.status) == vr.SEEDED)]
    assert np.array_equal(losses[k0].numpy(), mine[:7])
    points, sel = model.voxel_index.select(losses, max_points=10 ** 6)
    assert sorted(sel.cpu().tolist()) == sorted(keys.index(k) for k in losses)
    loss = model.calc_simi_loss(losses)
    assert loss is not None and bool(torch.isfinite(loss).all())
    # a model grown by a second sweep with new voxels keeps its ranges through prune + remap
    assert model.add_voxel_seeds(again) == (v, v + again.counts[4])
    drop = torch.zeros(model.P, dtype=torch.bool, device=dev)
    drop[::3] = True
    out = model.prune(min_opacity=0.0, max_scale=float("inf"), drop=drop)
    assert out["P_after"] == model.P == int((~drop).sum())
    rm = out["row_map"].tolist()
    for j, k in enumerate(keys):
        assert model.voxel_index.get(k) == (rm[j], 0 if j % 3 == 0 else 1)
    kept = [j for j in range(v) if j % 3]
    assert torch.equal(model._rotation.data[:len(kept)], seeds.rotation[kept])
    with pytest.raises(KeyError):
        model.add_voxel_seeds(seeds)                                             # a voxel seeds once
    with pytest.raises(ValueError):
        G.GrowableGaussians(16, 4, dev).add_voxel_seeds(G.SweepVoxelMap(0.25, 1, 0.001, capacity=64, device=dev)
                                                        .sweep(_t(pts[:5], dev)))
