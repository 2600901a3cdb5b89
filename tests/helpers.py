"""Shared helpers for the parity tests: numpy scene -> device tensors -> C ABI -> numpy."""
import numpy as np
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S


def to_dev(scene, dev):
    t = {}
    for k in ("bg", "means3D", "shs", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos",
              "colors_precomp", "cov3D_precomp"):
        v = scene.get(k)
        t[k] = torch.empty(0, device=dev) if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    return t


def hip_forward(scene, dev, debug=True, ref_rects=False, near_far=False):
    """ref_rects: binning mode of this forward (include/gsraster.h, gsr_set_reference_rects): True = the
    reference's own tile rectangles, False = the product's default culled ones.  near_far: allow the forward to bin
    the frame in a near and a far chain (gsr_set_near_far; the product's default -- off here because most tests
    compare the WHOLE per-tile lists with the oracle's).  Both are set for the CALLING THREAD only
    (gsr_set_*_thread): other rendering threads are not disturbed.  The thread's previous settings are restored."""
    t = to_dev(scene, dev)
    prev = G.set_reference_rects_thread(ref_rects)
    prev_nf = G.set_near_far_thread(near_far)
    try:
        out = G.rasterize_forward(t["bg"], t["means3D"], t["colors_precomp"], t["opacities"], t["scales"],
                                  t["rotations"], scene.get("scale_modifier", 1.0), t["cov3D_precomp"],
                                  t["viewmatrix"], t["projmatrix"], scene["tanfovx"], scene["tanfovy"], scene["H"],
                                  scene["W"], t["shs"], scene["sh_degree"], t["campos"], False, debug)
    finally:
        G.set_reference_rects_thread(prev)
        G.set_near_far_thread(prev_nf)
    return t, out


def hip_backward(scene, t, fwd, dL_dcolor, dL_dacc, dev, debug=True):
    R, color, depth, acc, radii, geom, binning, img = fwd
    dc = torch.from_numpy(dL_dcolor).to(dev)
    da = torch.from_numpy(dL_dacc).to(dev)
    g = G.rasterize_backward(t["bg"], t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"],
                             scene.get("scale_modifier", 1.0), t["cov3D_precomp"], t["viewmatrix"], t["projmatrix"],
                             scene["tanfovx"], scene["tanfovy"], dc, da, t["shs"], scene["sh_degree"], t["campos"],
                             geom, R, binning, img, debug, return_conic=True)
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations", "dL_dconic")
    return {n: x.cpu().numpy() for n, x in zip(names, g)}


def grad_close(got, ref, name, cond=None, outlier_frac=0.0, slack=None):
    """SURVEY.md Appendix B tolerance, |d| <= 1e-5 * max|g| + 1e-4 * |g|, with |g| taken as the largest
    component of the SAME Gaussian's gradient group (row): the f32 summation order differs from the
    oracle's, and the conic -> cov2D -> cov3D chain cancels large terms, so one component of a group can
    carry the rounding of its siblings (observed: inputs equal to 7 digits, one output off by 1.2e-4 rel).

    cond (stress scenes only): per-Gaussian condition number of the 2-D conic.  For needles (cond >> 1) every f32
    implementation -- the reference included -- loses digits in proportion to it: the power is a quadratic form
    whose terms cancel, and the backward inverts that matrix (backward.cu:140-275).  The oracle itself moves by
    more than the plain bound on such rows when only its summation order changes (tools/debug_random_scenes.py).
    With cond given, a row's bound is widened by (1 + cond / 10); 99.9 % of the elements must meet the widened
    bound and none may exceed it 20-fold.

    outlier_frac (full-size runs against the MULTI-THREADED oracle only): that oracle accumulates with f32 `omp atomic`
    adds in arbitrary order, as the reference's atomicAdd does, so its own result moves in the last bits from run to
    run; among 10^7 elements a handful then sit a hair outside the bound in some runs (observed: 1 of 12 M, 1.7e-6
    against a bound of 1.3e-6).  Up to this fraction may exceed the bound, none by more than 4x.

    slack (comparisons with the f64 restatement tests/ref64.py only): per element, how far the EXACT gradient moves
    when evaluated at the f32-rounded 2-D values an f32 backward is handed (ref64.render(..., slack=True)).  A row's
    bound is widened by its largest slack, so the row's factor 1 + slack / bound is computed in f64, row by row."""
    ref = ref.reshape(got.shape)
    if ref.size == 0:
        return
    P = ref.shape[0]
    scale = float(np.abs(ref).max())
    shape = (P,) + (1,) * (ref.ndim - 1)
    rowmax = np.abs(ref.reshape(P, -1)).max(1).reshape(shape)
    tol = 1e-5 * scale + 1e-4 * rowmax
    if slack is not None:
        tol = tol + np.abs(np.asarray(slack, np.float64)).reshape(P, -1).max(1).reshape(shape)
    if cond is not None:
        tol = tol * (1.0 + np.minimum(np.asarray(cond, np.float64), 1e6).reshape(shape) / 10.0)
    err = np.abs(got - ref)
    bad = err > tol
    msg = "%s: %d / %d outside tolerance, worst |d|=%.3e (max|g|=%.3e)" % (
        name, int(bad.sum()), bad.size, float(err.max()), scale)
    if cond is not None:
        assert bad.mean() <= 1e-3 and not (err > 20.0 * tol).any(), msg
    elif outlier_frac > 0.0:
        assert bad.mean() <= outlier_frac and not (err > 4.0 * tol).any(), msg
    else:
        assert not bad.any(), msg


def conic_condition(conic_opacity):
    """lambda_max / lambda_min of [[a, b], [b, c]] per Gaussian (inf where the conic is not positive definite)."""
    a, b, c = (np.asarray(conic_opacity[:, k], np.float64) for k in range(3))
    mid, det = 0.5 * (a + c), a * c - b * b
    disc = np.sqrt(np.maximum(mid * mid - det, 0.0))
    lo = mid - disc
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(lo > 0, (mid + disc) / lo, np.inf)
    return np.where(np.isfinite(k), k, 1e6)


def check_near_far_against_one_chain(sc, dev, near_entries, far_capacity=None, expect_redo=False, speculate_far=None):
    """One scene binned in one chain (the reference's structure) and near/far: observable results bit-identical, lists
    consistent (module docstring of include/gsraster.h, "Near/far frames")."""
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    G.set_binning_capacity_hint(0)
    t0, one = hip_forward(sc, dev, debug=False)                     # synchronous, one chain
    v1 = G.state_views(one[5], one[6], one[7], P, one[0], W, H)
    assert not v1["near_far"]
    assert torch.equal(v1["ranges_near"], v1["ranges"])             # one chain: the composed view is the raw one
    dcol, dacc = S.make_upstream_grads(W, H, 5)
    g1 = hip_backward(sc, t0, one, dcol, dacc, dev, debug=False)
    before = G.speculation_stats()
    G.set_near_far_hints(near_entries, far_capacity)
    if speculate_far is not None:   # True: this forward enqueues its far chain only once it has seen live tiles
        G.set_far_speculation(speculate_far)
    t1, two = hip_forward(sc, dev, debug=False, near_far=True)      # speculative, near/far
    bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x  # noqa: E731  (a NaN pixel equals itself)
    for i, (x, y) in enumerate(zip(one[1:5], two[1:5])):
        assert torch.equal(bits(x), bits(y)), i                     # colour, depth, silhouette, radii
    # host-side figures only now that the frame has completed: an asynchronous frame (far-chain speculation on a second
    # stream, include/gsraster.h) returns before its far chain's outcome is known and reports it once it is there
    torch.cuda.synchronize()
    far_skipped = G.last_far_skipped()
    st = G.speculation_stats()
    split, n_near, n_far = G.last_near_far()
    assert st["overflows"] - before["overflows"] == (1 if expect_redo else 0)
    assert split == (not expect_redo) and st["near_far_forwards"] == before["near_far_forwards"] + 1
    v2 = G.state_views(two[5], two[6], two[7], P, two[0], W, H)
    for k in ("n_contrib", "final_T", "quad_last", "tiles_touched"):
        assert torch.equal(bits(v1[k]), bits(v2[k])), k
    g2 = hip_backward(sc, t1, two, dcol, dacc, dev, debug=False)
    for k in g1:
        assert np.array_equal(g1[k], g2[k], equal_nan=True), k      # every gradient, bit for bit
    if expect_redo:
        assert int(two[0]) == int(one[0]) and torch.equal(v1["point_list"], v2["point_list"])
        return None
    assert v2["near_far"] and G.last_num_rendered() == n_near + n_far == v2["num_rendered"] <= int(one[0])
    assert int(two[0]) in (n_near, n_near + n_far)                  # (taken when the forward returned)
    # lists: per tile the near/far list is the one-chain list with far entries removed only where the tile was finished
    # by the near phase -- so its first max(n_contrib) entries, all that any pixel reads, are the same
    r1, r2 = v1["ranges"].long().cpu().numpy(), v2["ranges"].long().cpu().numpy()
    p1, p2 = v1["point_list"].cpu().numpy(), v2["point_list"].cpu().numpy()
    need = v1["quad_last"].long().max(1).values.cpu().numpy()
    rn, rf = v2["ranges_near"].long().cpu().numpy(), v2["ranges_far"].long().cpu().numpy()
    live = ~(v2["counters"][9] == 0)
    full_tiles = 0
    for tidx in range(r1.shape[0]):
        a, b = p1[r1[tidx, 0]:r1[tidx, 1]], p2[r2[tidx, 0]:r2[tidx, 1]]
        assert len(b) <= len(a) and np.array_equal(a[:need[tidx]], b[:need[tidx]]), tidx
        ln = rn[tidx, 1] - rn[tidx, 0]
        assert np.array_equal(a[:ln], b[:ln])                       # the near segment is a prefix of the whole list
        assert np.isin(b, a).all()
        full_tiles += int(len(a) == len(b))
    if speculate_far:   # completed without a far chain iff the near chain left no tile live
        assert far_skipped == (v2["counters"][9] == 0)
        assert st["far_skips"] - before["far_skips"] == int(far_skipped)
        assert st["far_skip_misses"] - before["far_skip_misses"] == int(not far_skipped)
    elif speculate_far is False:
        assert not far_skipped and st["far_skips"] == before["far_skips"]
    return dict(near=n_near, far=n_far, one=int(one[0]), live_tiles=v2["counters"][9], full_tiles=full_tiles,
                tiles=r1.shape[0], far_skipped=far_skipped)


GRAD_NAMES = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
              "dL_dscales", "dL_drotations")


def masked_upstream(W, H, seed, fragile):
    """make_upstream_grads with the fragile pixels zeroed (a cut decided within rounding distance may flip)."""
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    keep = (fragile == 0).astype(np.float32)
    return dcol * keep[None], dacc * keep[None]


def check_against_ref64(r, fragile, images=None, grads=None, cond=None):
    """An f32 frame (the oracle's or the HIP path's) against the f64 restatement r = ref64.render(..., slack=True):
    images <= 1e-4 off fragile pixels (depth relative to max(1, max depth), as check_forward), every gradient group
    within grad_close's bound widened per row by r['slack'] (and by the conic condition where cond is given).
    Returns {group: worst |d| / widened bound}."""
    ok = fragile == 0
    for name, got in (images or {}).items():
        ref = r[name]
        scale = max(1.0, float(np.abs(ref).max())) if name == "out_depth" else 1.0
        err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max(0)
        assert err[ok].max(initial=0) <= 1e-4 * scale, (name, float(err[ok].max()))
    worst = {}
    for k, got in (grads or {}).items():
        ref = r[k].reshape(np.shape(got))
        if ref.size == 0:
            continue
        grad_close(got, ref, k, cond=cond, slack=r["slack"][k])
        P = ref.shape[0]
        shape = (P,) + (1,) * (ref.ndim - 1)
        tol = 1e-5 * float(np.abs(ref).max()) + 1e-4 * np.abs(ref.reshape(P, -1)).max(1).reshape(shape)
        tol = tol + r["slack"][k].reshape(P, -1).max(1).reshape(shape)
        worst[k] = float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())
    return worst


# Scenes of the f64 comparisons (tests/test_ref64.py on the oracle, tests/test_gpu_ref64.py on the HIP path): the
# SCENES of test_gpu_parity.py plus one per path and per reference departure (tests/ref64.py, D1-D4)
REF64_SCENES = [(300, 70, 50, 11, 3), (1, 64, 64, 2, 0), (7, 33, 17, 3, 1), (2500, 257, 131, 4, 2),
                (10_000, 640, 480, 1, 0), (10_000, 640, 480, 1, 3), (40_000, 500, 300, 6, 1)]
REF64_PATHS = ("colors_precomp", "cov3D_precomp", "scale_modifier", "opaque", "jacobian_clamp", "sh_clamp")


def ref64_path_scene(kind, base=None):
    """(scene, seed) of one path of REF64_PATHS.  base(P, W, H, seed, D) builds the scene the path is laid over
    (default: S.make_scene; tests/intrinsics.py passes one with fx != fy)."""
    seed = {"colors_precomp": 13, "cov3D_precomp": 13, "scale_modifier": 14, "opaque": 15, "jacobian_clamp": 17,
            "sh_clamp": 18}[kind]
    D = 3 if kind == "sh_clamp" else 1
    sc = S.make_scene(1500, 200, 120, seed, sh_degree=D) if base is None else base(1500, 200, 120, seed, D)
    rng = np.random.default_rng(seed)
    if kind == "colors_precomp":
        sc["colors_precomp"] = rng.uniform(0, 1, (1500, 3)).astype(np.float32)
        sc["shs"] = None
    elif kind == "cov3D_precomp":
        from oracle import oracle as O
        base = O.forward(sc, keep_handle=False)
        cov = base.cov3D.copy()
        cov[base.radii <= 0] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32)
        sc["cov3D_precomp"] = cov
        sc["scales"] = None
        sc["rotations"] = None
    elif kind == "scale_modifier":  # D4; a black background drops the background term of dL_dalpha
        sc["scale_modifier"] = 0.7
        sc["bg"] = np.zeros(3, np.float32)
    elif kind == "opaque":  # D1: alpha = min(0.99, o G) saturates
        sc["opacities"][:300] = 1.0
        sc["opacities"][300:500] = 0.995
    elif kind == "jacobian_clamp":  # D3: big splats centred beyond 1.3 tanfov whose footprint reaches the image
        n = 60
        z = rng.uniform(1.5, 3.0, n)
        side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        k = rng.uniform(1.32, 1.6, n)
        horiz = rng.random(n) < 0.5
        m = np.zeros((n, 3))
        m[:, 2] = z
        m[:, 0] = np.where(horiz, side * k * sc["tanfovx"], rng.uniform(-0.5, 0.5, n) * sc["tanfovx"]) * z
        m[:, 1] = np.where(horiz, rng.uniform(-0.5, 0.5, n) * sc["tanfovy"], side * k * sc["tanfovy"]) * z
        sc["means3D"][:n] = m.astype(np.float32)
        sc["scales"][:n] = rng.uniform(0.12, 0.25, (n, 3)).astype(np.float32)
        sc["opacities"][:n] = rng.uniform(0.3, 0.8, (n, 1)).astype(np.float32)
    elif kind == "sh_clamp":  # colour = max(SH + 0.5, 0): a third of the Gaussians clamp in one channel
        ch = rng.integers(0, 3, 500)
        sc["shs"][np.arange(500), 0, ch] = rng.uniform(-3.0, -2.0, 500).astype(np.float32)
    return sc, seed
