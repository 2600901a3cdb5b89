"""GPU tests of sweep admission (csrc/seed.hip: gsr_sweep_admit; seed.py, model.py add_unexplained, torch_next.cpp).

Against float64 (tests/seed_ref.py, admit64): the reason codes, the six counts, the admitted rows and the continuous
outputs (z, the isotropic sigma^2, the colour) of every random case -- both image sizes (70 x 50, 33 x 17), posed
cameras, fx != fy, each optional input present and absent, radius 0 .. 3 -- each continuous output held to
max(2 e_ref, bar) with the bars counted in seed_ref's docstring and the fragile points removed from both sides (capped
at 1 % on the CPU, tests/test_seed_cases.py).  The exact cases compare bit for bit.  Every case prints its worst
|error| / bar; DESIGN.md section 2, "Sweep admission", is where they are recorded.

Exact properties: the compaction across workgroup seams (n = 1, 255, 256, 257, 1025; all, none and every other point
admitted), the per-pixel plane at H W = 1, 255, 257, every tensor and the workspace (exactly the queried size) at
0/4/8/12 bytes inside guarded allocations (tests/arena.py) with the rows at and behind the admitted count untouched,
agreement with gsr_lidar_depth_image (the shared projection), reproducibility bit for bit, a permuted sweep, the C++
route against the Python route, a refusal that writes nothing, and the end-to-end scene through
GrowableGaussians.add_unexplained."""
import ctypes as C

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import lidar_ref as L
import seed_ref as SR
from arena import PAT, Arena, offsets

pytestmark = pytest.mark.gpu
INF = float("inf")
OUTS = ("xyz", "covs_out", "rgb", "index", "pixel", "z")
WIDTH = dict(xyz=3, covs_out=9, rgb=3, index=1, pixel=1, z=1)


def _mat(a, n):
    return (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:n]])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _admit(dev, x, mode="a0", reasons=True, short=0, **scalars):
    """gsr_sweep_admit through ctypes, every device tensor and the workspace (exactly the queried size) inside guarded
    allocations prefilled with arena.PAT.  Returns (dict of copies: codes, counts, m, and the FULL-length outputs as
    int32 bit patterns), arena, return code."""
    lib = G.lib()
    n, H, W = int(x["points"].shape[0]), x["H"], x["W"]
    rows = max(n, 1)
    ar = Arena(dev, offsets(mode))
    put = lambda k, a: ar.put(k, torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev))  # noqa: E731
    put("points", x["points"])
    for k in ("covs", "depth", "acc", "lidar", "image", "exposure"):
        if x.get(k) is not None:
            put(k, x[k])
    for k in OUTS:
        if k != "rgb" or x.get("image") is not None:
            ar.put(k, shape=(rows, WIDTH[k]))
    ar.put("counts", shape=(6,))
    if reasons:
        ar.put("reasons", shape=((n + 3) // 4 + 1,))
    nbytes = int(lib.gsr_sweep_admit_workspace(n, H, W))
    assert nbytes % 4 == 0
    ar.put("ws", shape=(max(nbytes // 4, 1),))
    p = lambda k: C.c_void_p(ar.ptr(k)) if k in ar.t and ar.ptr(k) else None  # noqa: E731
    s = dict(acc_min=x["acc_min"], depth_tol=x["depth_tol"], occlusion_tol=x["occlusion_tol"], radius=x["radius"],
             footprint=x["footprint"], lo=x["min_depth"], hi=x["max_depth"], one=x["one_per_pixel"])
    s.update(scalars)
    rc = lib.gsr_sweep_admit(n, p("points"), p("covs"), _mat(x["T_cw"], 12), _mat(x["K"], 9), H, W, s["lo"], s["hi"],
                             p("depth"), p("acc"), s["acc_min"], s["depth_tol"], p("lidar"), int(s["radius"]),
                             s["occlusion_tol"], p("image"), p("exposure"), s["footprint"], int(bool(s["one"])),
                             p("xyz"), p("covs_out"), p("rgb"), p("index"), p("pixel"), p("z"), p("reasons"),
                             p("counts"), p("ws"), max(nbytes - short, 0), _stream())
    torch.cuda.synchronize()
    out = {k: ar.t[k].view(torch.int32).clone().cpu() for k in OUTS if k in ar.t}
    out["counts"] = ar.t["counts"].view(torch.int32).clone().cpu().numpy().astype(np.int64)
    out["m"] = int(out["counts"][0]) if rc == 0 else 0
    if reasons:
        out["codes"] = ar.t["reasons"].view(torch.uint8)[:n].clone().cpu().numpy()
    return out, ar, rc


def _got(out):
    """The admitted rows of _admit's copies as float / int arrays, in seed_ref.ratios' layout."""
    m = out["m"]
    f = lambda k: out[k][:m].view(torch.float32).numpy().astype(np.float64) if k in out else None  # noqa: E731
    return dict(codes=out.get("codes"), counts=out["counts"], index=out["index"][:m, 0].numpy(),
                pixel=out["pixel"][:m, 0].numpy(), z=f("z"), covs=f("covs_out"), rgb=f("rgb"), xyz=f("xyz"))


def _tail_untouched(out):
    return all(bool((out[k][out["m"]:] == PAT).all()) for k in OUTS if k in out)


def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in OUTS if k in a) and np.array_equal(a["counts"], b["counts"]) \
        and np.array_equal(a.get("codes"), b.get("codes"))


# ---- against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.CASE_NAMES)
def test_random_cases_against_float64(gpu_device, case):
    x, ref = SR.inputs(case), SR.reference(case)
    out, ar, rc = _admit(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None and _tail_untouched(out)
    assert int(out["counts"].sum()) == x["n"]
    assert np.array_equal(np.bincount(out["codes"], minlength=6), out["counts"])
    g = _got(out)
    r = SR.ratios(g, ref, x)
    print(case, "counts", out["counts"], "fragile", ref["n_fragile"], "ratios", r)
    assert r["codes"] == 0 and r["rows"] and r["counts"] <= 1.0
    for k in ("z", "var", "rgb"):
        assert r.get(k, 0.0) <= 1.0, (case, k, r[k])
    t = ref["truth"]
    pts32 = torch.from_numpy(x["points"]).view(torch.int32)
    assert torch.equal(out["xyz"][:out["m"]], pts32[torch.from_numpy(g["index"]).long()])     # the input bits
    if x["covs"] is not None:
        cov32 = torch.from_numpy(x["covs"]).view(torch.int32)
        assert torch.equal(out["covs_out"][:out["m"]], cov32[torch.from_numpy(g["index"]).long()])
    else:
        off = g["covs"][:, [1, 2, 3, 5, 6, 7]]
        assert (off == 0).all() and not np.signbit(off).any()
        assert np.array_equal(g["covs"][:, 0], g["covs"][:, 4]) and np.array_equal(g["covs"][:, 0], g["covs"][:, 8])
    assert t["counts"].sum() == x["n"]


@pytest.mark.parametrize("case", SR.EXACT_NAMES)
def test_exact_cases_bit_for_bit(gpu_device, case):
    x, t = SR.inputs(case), SR.reference(case)["truth"]
    out, ar, rc = _admit(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None and _tail_untouched(out)
    g = _got(out)
    assert np.array_equal(out["counts"], t["counts"]) and np.array_equal(out["codes"], t["codes"])
    assert np.array_equal(g["index"], t["index"]) and np.array_equal(g["pixel"], t["pixel"])
    for k, want in (("z", t["z"]), ("covs", t["covs"]), ("rgb", t["rgb"]), ("xyz", t["xyz"])):
        assert np.array_equal(g[k].reshape(np.asarray(want).shape), np.asarray(want, np.float64)), (case, k)
    if x["n"]:
        assert tuple(int(c) for c in out["codes"][-len(SR.EXACT_SPECIAL_CODES):]) == SR.EXACT_SPECIAL_CODES


# ---- seams -------------------------------------------------------------------------------------------------------------
def _lattice(n, pattern, H=50, W=70):
    """n dyadic points, point i alone in pixel i (row-major) at z == 2, under the exact camera; `pattern` decides which
    of them are in view: the others lie behind the camera."""
    K = L.EXACT_K
    i = np.arange(n)
    on = dict(all=np.ones(n, bool), none=np.zeros(n, bool), alternating=i % 2 == 0)[pattern]
    z = np.where(on, 2.0, -2.0)
    pts = np.stack([((i % W) - K[0, 2]) / K[0, 0] * z, ((i // W) - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)
    covs = np.random.default_rng(n).uniform(0.1, 1.0, (n, 9)).astype(np.float32)
    x = dict(points=pts, T_cw=L.EXACT_T, K=K, H=H, W=W, n=n, min_depth=0.25, max_depth=8.0, acc_min=0.5,
             depth_tol=0.5, occlusion_tol=0.25, radius=1, footprint=1.0, one_per_pixel=True, covs=covs)
    return x, np.nonzero(on)[0]


@pytest.mark.parametrize("pattern", ("all", "none", "alternating"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 4 * 256 + 1))
def test_compaction_seams(gpu_device, n, pattern):
    x, want = _lattice(n, pattern)
    out, ar, rc = _admit(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None and _tail_untouched(out)
    m = out["m"]
    assert m == len(want) and out["counts"][1] == n - m and int(out["counts"].sum()) == n
    idx = out["index"][:m, 0].numpy()
    assert np.array_equal(idx, want) and (np.diff(idx) > 0).all()
    sel = torch.from_numpy(want).long()
    assert torch.equal(out["xyz"][:m], torch.from_numpy(x["points"]).view(torch.int32)[sel])
    assert torch.equal(out["covs_out"][:m], torch.from_numpy(x["covs"]).view(torch.int32)[sel])
    assert np.array_equal(out["pixel"][:m, 0].numpy(), want)
    assert (out["z"][:m].view(torch.float32) == 2.0).all()


@pytest.mark.parametrize("shape", ((1, 1), (15, 17), (1, 257)))
def test_plane_seams(gpu_device, shape):
    """H W = 1, 255 and 257: the per-pixel plane on both sides of a workgroup of pixels, several points per pixel."""
    H, W = shape
    rng = np.random.default_rng(H * W)
    n, K = 300, L.EXACT_K
    X, Y = rng.integers(-2, 4 * W + 2, n) / 4.0, rng.integers(-2, 4 * H + 2, n) / 4.0
    z = rng.choice([1.0, 1.25, 2.0, 4.0], n)
    pts = np.stack([(X - K[0, 2]) / K[0, 0] * z, (Y - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)
    x = dict(points=pts, T_cw=L.EXACT_T, K=K, H=H, W=W, n=n, min_depth=0.25, max_depth=8.0, acc_min=0.5, depth_tol=0.5,
             occlusion_tol=0.25, radius=1, footprint=1.5, one_per_pixel=True)
    t = SR.admit64(x)
    out, ar, rc = _admit(gpu_device, x)
    assert rc == 0, G.lib().gsr_last_error()
    assert ar.guards_intact() is None and _tail_untouched(out)
    g = _got(out)
    assert np.array_equal(out["codes"], t["codes"]) and np.array_equal(out["counts"], t["counts"])
    assert np.array_equal(g["index"], t["index"]) and np.array_equal(g["pixel"], t["pixel"])
    assert np.array_equal(g["z"][:, 0], t["z"]) and np.array_equal(g["covs"], t["covs"])
    assert t["counts"][SR.DUPLICATE] > 0 and out["m"] <= H * W


# ---- placement, reproducibility, permutation -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("a4", "a8", "a12", "mix"))
def test_guarded_buffers_at_every_offset(gpu_device, mode):
    for case in ("full_70x50", "posed_70x50"):
        x = SR.inputs(case)
        base, ar0, rc0 = _admit(gpu_device, x, "a0")
        out, ar, rc = _admit(gpu_device, x, mode)
        assert rc0 == 0 and rc == 0, G.lib().gsr_last_error()
        assert ar0.guards_intact() is None and ar.guards_intact() is None
        assert _tail_untouched(out) and _tail_untouched(base) and 0 < out["m"] < x["n"]
        assert _same_bits(base, out)


def test_two_runs_give_the_same_bits(gpu_device):
    x = SR.inputs("full_70x50")
    a, _, _ = _admit(gpu_device, x)
    b, _, _ = _admit(gpu_device, x)
    assert a["m"] > 0 and _same_bits(a, b)
    c, _, _ = _admit(gpu_device, x, reasons=False)      # the nullable reasons change nothing else
    assert all(torch.equal(a[k], c[k]) for k in OUTS) and np.array_equal(a["counts"], c["counts"])


@pytest.mark.parametrize("case", ("full_70x50", "all_per_pixel_70x50"))
def test_a_permuted_sweep_admits_the_same_points(gpu_device, case):
    x = SR.inputs(case)
    a, _, _ = _admit(gpu_device, x)
    perm = np.random.default_rng(5).permutation(x["n"])
    b, _, _ = _admit(gpu_device, dict(x, points=x["points"][perm]))
    assert np.array_equal(a["counts"], b["counts"])
    assert np.array_equal(np.sort(perm[b["index"][:b["m"], 0].numpy()]), a["index"][:a["m"], 0].numpy())
    assert np.array_equal(b["codes"], a["codes"][perm])


# ---- the shared projection -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("full_70x50", "posed_70x50", "tiny_33x17"))
def test_agrees_with_the_lidar_image(gpu_device, case):
    x = SR.inputs(case)
    pts = torch.from_numpy(x["points"]).to(gpu_device)
    image, counts2 = G.lidar_depth_image(pts, x["T_cw"], x["K"], x["H"], x["W"], x["min_depth"], x["max_depth"],
                                         want_counts=True)
    a = G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=0.05, occlusion_tol=0.1,
                      min_depth=x["min_depth"], max_depth=x["max_depth"], one_per_pixel=True)
    counts2 = counts2.tolist()
    assert a.counts[0] == counts2[1] == a.index.numel()          # one admitted point per pixel hit
    assert a.counts[1] == x["n"] - counts2[0]
    assert a.counts[2] == a.counts[3] == a.counts[4] == 0 and sum(a.counts) == x["n"]
    assert torch.equal(a.z.view(torch.int32), image.reshape(-1)[a.pixel.long()].view(torch.int32))
    assert a.rgbs is None and a.reasons is None


# ---- the routes ----------------------------------------------------------------------------------------------------------
def _kwargs(x, dev):
    t = lambda k: None if x.get(k) is None else torch.from_numpy(x[k]).to(dev)  # noqa: E731
    return dict(depth=t("depth"), acc=t("acc"), image=t("image"), lidar_depth=t("lidar"), covs=t("covs"),
                exposure=t("exposure"), acc_min=x["acc_min"], occlusion_radius=x["radius"], footprint=x["footprint"],
                min_depth=x["min_depth"], max_depth=x["max_depth"], one_per_pixel=x["one_per_pixel"], want_reasons=True)


@pytest.mark.parametrize("case", ("full_70x50", "posed_70x50", "no_lidar_33x17", "exact_n0"))
def test_python_route_and_cpp_route(gpu_device, case):
    x = SR.inputs(case)
    base, _, _ = _admit(gpu_device, x)
    pts = torch.from_numpy(x["points"]).to(gpu_device)
    kw = _kwargs(x, gpu_device)
    a = G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=x["depth_tol"], occlusion_tol=x["occlusion_tol"],
                      **kw)
    nx = G.torch_ops().next
    b = nx.admit_sweep(pts, torch.from_numpy(np.asarray(x["T_cw"], np.float32)), torch.from_numpy(np.asarray(x["K"], np.float32)),
                       x["H"], x["W"], x["depth_tol"], x["occlusion_tol"], **kw)
    m = base["m"]
    assert a.counts == tuple(base["counts"]) == tuple(b[6]) and a.xyz.shape == (m, 3) and a.covs.shape == (m, 3, 3)
    bits = lambda v: v.reshape(m, WIDTH[k]).view(torch.int32).cpu()  # noqa: E731
    for k, mine, theirs in (("xyz", a.xyz, b[0]), ("covs_out", a.covs, b[1]), ("rgb", a.rgbs, b[2]),
                            ("index", a.index, b[3]), ("pixel", a.pixel, b[4]), ("z", a.z, b[5])):
        if mine is None:
            assert theirs is None and k not in base
            continue
        assert torch.equal(bits(mine), base[k][:m]) and torch.equal(bits(theirs), base[k][:m]), (case, k)
    assert np.array_equal(a.reasons.cpu().numpy(), base["codes"]) and np.array_equal(b[7].cpu().numpy(), base["codes"])


def test_log_gain_and_shared_exposure(gpu_device):
    x = SR.inputs("full_70x50")
    pts = torch.from_numpy(x["points"]).to(gpu_device)
    img = torch.from_numpy(x["image"]).to(gpu_device)
    run = lambda e, lg: G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=0.05, occlusion_tol=0.1,  # noqa: E731
                                      image=img, exposure=e, log_gain=lg).rgbs
    shared = torch.tensor([0.25, 0.1], device=gpu_device)
    rows = torch.stack([torch.exp(shared[0]), shared[1]]).expand(3, 2).contiguous()
    assert torch.equal(run(shared, True), run(rows, False))
    plain = run(None, False)
    assert torch.allclose(run(rows, False), (plain / 255 - 0.1) / float(torch.exp(shared[0])) * 255, rtol=1e-5, atol=1e-2)


def test_refusals_write_nothing(gpu_device):
    x = SR.inputs("full_70x50")
    for kw in (dict(short=1), dict(radius=4), dict(depth_tol=-1.0), dict(acc_min=0.0), dict(hi=0.1)):
        out, ar, rc = _admit(gpu_device, x, **kw)
        assert rc == -1, kw
        assert ar.guards_intact() is None
        assert all(bool((out[k] == PAT).all()) for k in OUTS) and bool((ar.t["counts"].view(torch.int32) == PAT).all())
        assert bool((ar.t["reasons"].view(torch.int32) == PAT).all()) and bool((ar.t["ws"].view(torch.int32) == PAT).all())
    pts = torch.from_numpy(x["points"]).to(gpu_device)
    with pytest.raises(G.GsrError, match="bad occlusion_radius"):
        G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=0.05, occlusion_tol=0.1, occlusion_radius=7)
    with pytest.raises(G.GsrError, match="depth and acc"):
        G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=0.05, occlusion_tol=0.1,
                      depth=torch.zeros((x["H"], x["W"]), device=gpu_device))
    with pytest.raises(G.GsrError, match="bad footprint"):
        G.admit_sweep(pts, x["T_cw"], x["K"], x["H"], x["W"], depth_tol=0.05, occlusion_tol=0.1, footprint=-1.0)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_add_unexplained_closes_the_hole(gpu_device):
    """The three conditions of tests/test_seed_cases.py's end-to-end case on HIP renders, through
    GrowableGaussians.add_unexplained; the rows that were there keep their bits, Adam moments included."""
    import iteration as IT
    dev = gpu_device
    s = SR.hole_scene()
    H, W = s["H"], s["W"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    model = G.GrowableGaussians(1024, 4, dev)
    opt = G.GrowableAdam(model)
    P0 = s["xyz"].shape[0]
    assert model.add_new_pointcloud(t(s["xyz"]), torch.diag_embed(t(s["scales"]) ** 2), t(s["rgbs"]), 1.0) == (0, P0)
    cam = G.Camera(np.eye(3), np.zeros(3), IT.FOVX, IT.FOVY, W, H, device=dev)
    bg = torch.zeros(3, device=dev)
    sweep = t(s["sweep"])
    for name in model._NAMES:           # moments that are not zero, so that "kept their bits" says something
        model._m[name][:P0].uniform_(-1, 1)
        model._v[name][:P0].uniform_(0, 1)
    before = {n: [b[n][:P0].clone() for b in (model._buf, model._m, model._v)] for n in model._NAMES}

    def render():
        with torch.no_grad():
            color, depth, acc = G.render(cam, model, bg)
        return color.clamp(0, 1), depth, acc

    color, depth, acc = render()
    lidar = G.lidar_depth_image(sweep, G.world_to_camera(cam), G.raster_K(W, H, IT.FOVX, IT.FOVY), H, W)
    hit = (lidar.reshape(-1) > 0).cpu().numpy() & SR.in_hole(np.arange(H * W), W)
    assert (acc.reshape(-1).cpu().numpy()[hit] < SR.E2E["acc_min"]).mean() >= 0.5       # it is a hole
    lo, hi, counts = model.add_unexplained(sweep, cam, depth, acc, color, **SR.E2E)
    m1 = counts[0]
    assert (lo, hi) == (P0, P0 + m1) and model.P == hi and sum(counts) == sweep.shape[0]
    a = G.admit_sweep(sweep, G.world_to_camera(cam), G.raster_K(W, H, IT.FOVX, IT.FOVY), H, W, depth=depth, acc=acc,
                      image=color, **SR.E2E)
    assert a.counts == counts and torch.equal(model._buf["_xyz"][lo:hi], a.xyz)
    inside = SR.in_hole(a.pixel.cpu().numpy(), W).mean()
    color2, depth2, acc2 = render()
    closed = (acc2.reshape(-1).cpu().numpy()[hit] >= SR.E2E["acc_min"]).mean()
    again = G.admit_sweep(sweep, G.world_to_camera(cam), G.raster_K(W, H, IT.FOVX, IT.FOVY), H, W, depth=depth2,
                          acc=acc2, image=color2, **SR.E2E).counts[0]
    print("admitted", m1, "in the hole", inside, "closed", closed, "second admission", again)
    assert m1 >= 200 and inside >= 0.9 and closed >= 0.9 and again <= 0.1 * m1
    for n in model._NAMES:
        for was, b in zip(before[n], (model._buf, model._m, model._v)):
            assert torch.equal(was.view(torch.int32), b[n][:P0].view(torch.int32)), n
        assert not bool(model._m[n][lo:hi].any()) and not bool(model._v[n][lo:hi].any())   # the new rows start at zero
    assert opt is not None
