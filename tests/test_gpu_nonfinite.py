"""GPU tests (run with -m gpu on an MI355X): the HIP path ON its cull boundaries and on non-finite Gaussians, against
the outcomes tests/nonfinite.py writes out from the reference's source lines and against the CPU oracle.

Every other GPU module draws its inputs from continuous ranges: a kernel that culls on `pvz < 0.2f`, `s >= 0.3f`,
`alpha <= 1/255` or `power >= 0`, that propagates a NaN through the 0.99 clamp, or that counts the duplicate lanes of the
last k_preprocess block passes all of them.  The scenes here are small (two Gaussians at 33 x 17, 300 at 65 x 49): the
decisions are per Gaussian and per pixel, there is nothing a larger frame would add.
"""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
import nonfinite as NF
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, check_near_far_against_one_chain, grad_close, hip_forward, to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu
IMG_TOL, FRAGILE_TOL = 1e-4, 2e-2       # the bars of tests/test_gpu_parity.py
MODES = ("reference", "culled")
BWD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations", "dL_dconic", "dL_ddepths")


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _close(got, ref, tol, what):
    """|got - ref| <= tol where ref is finite; where it is not, got is the same NaN / Inf."""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    assert NF.same(got[~fin], ref[~fin]), what
    assert np.isfinite(got[fin]).all(), what
    assert np.abs(got[fin] - ref[fin]).max(initial=0) <= tol, (what, float(np.abs(got[fin] - ref[fin]).max()))


def check_forward(sc, fr, fwd, debug=True, max_fragile=5e-3):
    """The stages of test_gpu_parity.check_forward with NaN equal to NaN: integer stages bit-exact, per-Gaussian records
    of every row that has a radius OR a tile, images within 1e-4 off fragile pixels.  max_fragile None (boundary scenes):
    EVERY pixel is held to the tight bars, whatever the fragile map says.  Pixels whose flag has bit 1 set -- an opacity
    of -Inf times an exp(power) in the subnormal range, decided by the exp implementation alone -- may flip by a whole
    0.99 T and are not compared; they count towards max_fragile like the others."""
    R, color, depth, acc, radii, geom, binning, img = fwd
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    assert R == fr.R
    v = G.state_views(geom, binning, img, P, R, W, H)
    assert v["num_rendered"] == fr.R
    assert np.array_equal(radii.cpu().numpy(), fr.radii)
    assert np.array_equal(_u32(v["tiles_touched"]), fr.tiles_touched)
    if debug:
        assert np.array_equal(_u32(v["point_offsets"]), fr.point_offsets)
    vis = (fr.radii > 0) | (fr.tiles_touched > 0)
    sp = v["splats"].cpu().numpy()
    assert NF.same(sp[vis, 0:2], fr.means2D[vis])
    assert NF.same(sp[vis, 9], fr.depths[vis]) and NF.same(v["depths"].cpu().numpy()[vis], fr.depths[vis])
    assert NF.same(sp[vis][:, 2:5], fr.conic_opacity[vis][:, :3])
    assert NF.same(sp[vis, 5], fr.conic_opacity[vis, 3])
    if sc.get("colors_precomp") is None:
        _close(sp[vis, 6:9], fr.rgb[vis], 1e-6, "rgb")
        cl = v["clamped"].cpu().numpy()
        assert np.array_equal(np.stack([(cl >> k) & 1 for k in range(3)], 1)[vis], fr.clamped[vis])
    if sc.get("cov3D_precomp") is None and debug:
        # bit-equal where the reference's covariance is finite; where it is not, not finite here either.  (Not "the
        # same NaN / Inf": k_preprocess forms M = S R without the structural zeros of S, so an infinite rotation entry
        # stays +-Inf where GLM's full product has 0 * Inf = NaN.  Both end in the same NaN conic, compared above.)
        got, ref = v["cov3D"].cpu().numpy()[vis], fr.cov3D[vis]
        fin = np.isfinite(ref).all(1)
        assert np.array_equal(got[fin], ref[fin]) and not np.isfinite(got[~fin]).all(1).any()
    if R:
        assert np.array_equal(v["keys"].cpu().numpy().view(np.uint64), fr.keys)
        assert np.array_equal(_u32(v["point_list"]), fr.point_list)
    assert np.array_equal(_u32(v["ranges"]), fr.ranges)
    frag = fr.fragile > 0
    skip = (fr.fragile & 2) > 0
    if max_fragile is None:
        frag = np.zeros_like(frag)
        assert not skip.any()
    else:
        assert frag.mean() < max_fragile
    assert np.array_equal(_u32(v["n_contrib"])[~frag], fr.n_contrib[~frag])
    frag = frag & ~skip
    for name, got, ref in (("color", color, fr.out_color), ("depth", depth, fr.out_depth), ("acc", acc, fr.out_acc),
                           ("final_T", v["final_T"][None], fr.final_T[None])):
        got = got.cpu().numpy()
        fin = np.isfinite(ref).all(0)
        scale = max(1.0, float(np.abs(ref[:, fin]).max(initial=0))) if name == "depth" else 1.0
        _close(got[:, ~frag & ~skip], ref[:, ~frag & ~skip], IMG_TOL * scale, name)
        _close(got[:, frag], ref[:, frag], FRAGILE_TOL * scale, name + " (fragile)")
    return v


def _backward(sc, t, fwd, dcol, dacc, dev, depth, debug=True):
    """gsr_backward, or gsr_backward_depth with a zero dL_ddepth (the DEPTH instantiations of both backward kernels; the
    nine groups are then the plain backward's)."""
    R, _, _, _, radii, geom, binning, img = fwd
    dc, da = torch.from_numpy(dcol).to(dev), torch.from_numpy(dacc).to(dev)
    g = G.rasterize_backward(t["bg"], t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"],
                             sc.get("scale_modifier", 1.0), t["cov3D_precomp"], t["viewmatrix"], t["projmatrix"],
                             sc["tanfovx"], sc["tanfovy"], dc, da, t["shs"], sc["sh_degree"], t["campos"], geom, R,
                             binning, img, debug, return_conic=True, grad_depth=torch.zeros_like(da) if depth else None)
    return {n: x.cpu().numpy() for n, x in zip(BWD_NAMES, g)}


def finite_rows(g, P):
    """rows all of whose nine groups are finite"""
    fin = np.ones(P, bool)
    for k in GRAD_NAMES:
        if g[k].size:
            fin &= np.isfinite(g[k].reshape(P, -1)).all(1)
    return fin


def check_gradients(got, ref, P):
    """grad_close on the rows the oracle has finite -- a row counts as finite when every one of its nine groups is; its
    max|g| runs over the array it is given, so the other rows are taken out first -- and every such row is finite on
    the HIP side (test_rows_the_oracle_has_finite_are_finite_here reports the rows when that fails).
    (A poisoned row that keeps radii == 0 gets exact zeros from the library where the oracle's blend backward leaves a
    finite dL_dcolors next to its NaN dL_dmeans2D: the row is out either way.)"""
    fin = finite_rows(ref, P)
    assert fin.sum() > P // 2 and finite_rows(got, P)[fin].all()
    for k in GRAD_NAMES:
        r = ref[k]
        if r.size:
            grad_close(got[k].reshape(r.shape)[fin], r[fin], k)


# ---- boundaries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(NF.BOUNDARIES))
def test_boundary(name, mode, gpu_device):
    dev = gpu_device
    sc, ex = NF.BOUNDARIES[name]()
    O.set_threads(1)
    fr = O.forward(sc, tight=(mode == "culled"))
    t, dbg = hip_forward(sc, dev, debug=True, ref_rects=(mode == "reference"))
    v = check_forward(sc, fr, dbg, max_fragile=None)
    _, prod = hip_forward(sc, dev, debug=False, ref_rects=(mode == "reference"))
    assert int(prod[0]) == int(dbg[0])
    for i in (1, 2, 3, 4):                                   # colour, depth, silhouette, radii: bit for bit
        assert torch.equal(_bits(dbg[i]), _bits(prod[i])), i
    # the outcome, from the reference's source line (tests/nonfinite.py)
    vis = np.array(ex["visible"])
    radii = dbg[4].cpu().numpy()
    tiles = _u32(v["tiles_touched"])
    assert np.array_equal(radii > 0, vis) and not tiles[~vis].any()
    if not (name == "alpha_out" and mode == "culled"):
        assert (tiles[vis] > 0).all()
    px = dbg[1][:, NF.CY, NF.CX].cpu().numpy()
    nc = int(_u32(v["n_contrib"])[NF.CY, NF.CX])
    fT = v["final_T"][NF.CY, NF.CX].item()
    assert nc == int(fr.n_contrib[NF.CY, NF.CX])
    dcol, dacc = NF.centre_upstream()
    for depth in (False, True):
        g = _backward(sc, t, dbg, dcol, dacc, dev, depth)
        if name == "alpha_in":
            assert g["dL_dopacity"][0, 0] != 0
        if name == "alpha_out":
            assert g["dL_dopacity"][0, 0] == 0 and not any(x.any() for x in g.values())
        with np.errstate(all="ignore"):
            _boundary_gradients(g, O.backward(fr, sc, dcol, dacc), len(vis))
    if name == "alpha_in":
        assert nc == 1 and np.abs(px - ex["centre"]).max() <= IMG_TOL and not np.array_equal(px, NF.BG)
    if name == "alpha_out":
        assert nc == 0 and np.array_equal(px, NF.BG) and fT == 1.0
        assert torch.equal(dbg[1].cpu(), torch.from_numpy(NF.BG)[:, None, None].expand(3, NF.H0, NF.W0))
    if name == "alpha_clamp":
        assert nc == 1 and np.float32(fT) == ex["final_T"]


def _boundary_gradients(got, ref, P):
    """every row of a boundary scene is finite: all of them, all nine groups"""
    for k in GRAD_NAMES:
        if ref[k].size:
            assert np.isfinite(ref[k]).all(), k
            grad_close(got[k].reshape(ref[k].shape), ref[k], k)


def _bits(x):
    return x.view(torch.int32) if x.is_floating_point() else x


# ---- poisoned scenes ---------------------------------------------------------------------------------------------
def _poison_cases():
    out = []
    for D in (0, 3):
        out += [(D,) + c for c in NF.cases(D)] + [(D, "everything", "", ())]
    return out


def _ids(c):
    return "D%d-%s-%s-%s" % (c[0], c[1], c[2], "all" if len(c[3]) > 1 else "".join(map(str, c[3])))


def _scene(D, field, value, rows):
    return NF.everything(D) if field == "everything" else NF.poisoned(D, field, value, rows)


@pytest.mark.parametrize("case", _poison_cases(), ids=_ids)
def test_poisoned_scene_against_the_oracle(case, gpu_device):
    """Every stage of the forward bit-exact or within 1e-4, in both binning modes, through the debug forward and the
    product forward (at degree 3 the pipelined SH-row variant, whose last block's duplicate lanes re-evaluate row
    P - 1); the nine gradient groups on the rows the oracle has finite, with and without the depth gradient."""
    dev = gpu_device
    sc, clean, rows = _scene(*case)
    O.set_threads(1)
    dcol, dacc = S.make_upstream_grads(NF.PW, NF.PH, NF.SEED)
    for mode in MODES:
        fr = O.forward(sc, tight=(mode == "culled"))
        keep = (fr.fragile == 0).astype(np.float32)
        with np.errstate(all="ignore"):
            ref = O.backward(fr, sc, dcol * keep, dacc * keep)
        for debug in (True, False):
            t, fwd = hip_forward(sc, dev, debug=debug, ref_rects=(mode == "reference"))
            check_forward(sc, fr, fwd, debug=debug)
            for depth in (False, True):
                got = _backward(sc, t, fwd, dcol * keep, dacc * keep, dev, depth, debug=debug)
                check_gradients(got, ref, NF.PP)


@pytest.mark.parametrize("case", _poison_cases(), ids=_ids)
def test_rows_the_oracle_has_finite_are_finite_here(case, gpu_device):
    """Every row whose gradients the oracle has finite must be finite on the HIP side.  Two things this holds in the
    blend backward (both were wrong before this test existed):
      * an opacity of -Inf on a row ALL of whose pixels skip it: the reference adds nothing to the row, so its gradient
        is 0 -- k_gather_records must not turn the row's zero sums into 0 * -Inf = NaN when it applies the opacity;
      * a non-finite COLOUR on a splat that a pixel SKIPS: the per-quad kernel runs skipped lanes with alpha = 0, and
        alpha * (colour . dL/dpixel - S) must not put 0 * Inf = NaN into S, the recurrence of everything behind the next
        splat -- the reference's accum_rec only ever sees splats the pixel blended."""
    dev = gpu_device
    sc, clean, rows = _scene(*case)
    O.set_threads(1)
    dcol, dacc = S.make_upstream_grads(NF.PW, NF.PH, NF.SEED)
    for mode in MODES:
        fr = O.forward(sc, tight=(mode == "culled"))
        keep = (fr.fragile == 0).astype(np.float32)
        with np.errstate(all="ignore"):
            ref = O.backward(fr, sc, dcol * keep, dacc * keep)
        t, fwd = hip_forward(sc, dev, debug=False, ref_rects=(mode == "reference"))
        got = _backward(sc, t, fwd, dcol * keep, dacc * keep, dev, False, debug=False)
        extra = np.flatnonzero(finite_rows(ref, NF.PP) & ~finite_rows(got, NF.PP))
        print("%s %s: non-finite here, finite in the oracle: %d rows (%d of them poisoned), oracle non-finite: %d"
              % (_ids(case), mode, extra.size, int(np.isin(extra, rows).sum()), int((~finite_rows(ref, NF.PP)).sum())))
        assert extra.size == 0, (mode, extra.tolist(), sorted(rows))


def test_near_far_split_of_the_all_poisons_scene(gpu_device):
    sc, _, _ = NF.everything(0)
    try:
        st = check_near_far_against_one_chain(sc, gpu_device, 1)
        assert st["near"] > 0 and st["far"] > 0
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


def test_mark_visible_with_nonfinite_means(gpu_device):
    sc = NF.base(0)
    m = sc["means3D"].copy()
    m[0, 2], m[1, 2], m[2, 2], m[3, 0], m[4, 1], m[5, 2], m[6, 2] = (np.nan, np.inf, -np.inf, np.nan, np.inf,
                                                                     np.float32(0.2), NF.up(0.2))
    m[NF.PP - 1, 2] = np.nan
    t = to_dev(dict(sc, means3D=m), gpu_device)
    got = G.mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"]).cpu().numpy()
    want = O.mark_visible(m, sc["viewmatrix"])
    assert np.array_equal(got, want) and want[:7].tolist() == [True, True, False, True, True, False, True]


# ---- the autograd surface and the prune ------------------------------------------------------------------------------
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def _model(sc, dev, rows=None):
    """A GrowableGaussians holding the scene's rows (all, or `rows`) as raw leaves."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sel = slice(None) if rows is None else rows
    op = tt(sc["opacities"][sel]).double()
    L = {"_xyz": tt(sc["means3D"][sel]), "_features_dc": tt(sc["shs"][sel][:, :1]),
         "_features_rest": tt(sc["shs"][sel][:, 1:]), "_scaling": torch.log(tt(sc["scales"][sel])),
         "_rotation": tt(sc["rotations"][sel]) * 1.7, "_opacity": torch.log(op / (1 - op)).float()}
    P, M = L["_xyz"].shape[0], sc["shs"].shape[1]
    m = G.GrowableGaussians(P + 64, M, dev)
    for n in LEAVES:
        m._buf[n][:P].copy_(L[n])
    m.P = P
    m._bind()
    m.fused_tail = False
    return m


@pytest.mark.parametrize("D", [0, 3])
def test_render_of_a_model_with_a_nan_scale_row_and_its_prune(D, gpu_device):
    """One raw scale of one row is NaN (one bad Adam step).  The row is NOT dead to the rasterizer: it has radius 0 and
    paints its tile at alpha 0.99.  Every other row still gets finite gradients; prune() drops the row, and the frame
    afterwards is, bit for bit, the frame of a model built from the surviving rows -- and not the frame before."""
    dev, W, H = gpu_device, NF.PW, NF.PH
    sc = NF.base(D)
    bad = NF.DIAGONAL_ROW
    settings = G.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], torch.from_numpy(sc["bg"]).to(dev),
                                               1.0, torch.from_numpy(sc["viewmatrix"]).to(dev),
                                               torch.from_numpy(sc["projmatrix"]).to(dev), D,
                                               torch.from_numpy(sc["campos"]).to(dev), False, False)
    gen = torch.Generator().manual_seed(6)
    wc, wa = (torch.randn(s, generator=gen).to(dev) for s in ((3, H, W), (1, H, W)))

    def render(m, backward=True):
        xyz, opac, scales, rot, shs = m.activated()
        color, radii, depth, acc = G.GaussianRasterizer(settings)(xyz, torch.zeros_like(xyz), opac, shs=shs, scales=scales,
                                                                 rotations=rot)
        if backward:
            ((color * wc).sum() + (acc * wa).sum()).backward()
        return color.detach(), depth.detach(), acc.detach(), radii

    prev = G.set_near_far_thread(False)
    try:
        m = _model(sc, dev)
        with torch.no_grad():
            m._scaling[bad, 1] = float("nan")
        m._next_act = None
        c0, d0, a0, r0 = render(m)
        finite = torch.ones(NF.PP, dtype=torch.bool, device=dev)
        finite[bad] = False
        for n in LEAVES:
            g = getattr(m, n).grad
            if g is not None and g.numel():
                assert bool(torch.isfinite(g[finite]).all()), n
        assert bool(torch.isfinite(m._xyz.grad[finite]).all()) and bool(m._xyz.grad[finite].any())
        assert int(r0[bad]) == 0 and bool(torch.isfinite(c0).all())
        out = m.prune()
        keep = out["reasons"] == 0
        assert out["n_nonfinite"] == 1 and not bool(keep[bad]) and m.P == int(keep.sum())
        c1, d1, a1, r1 = render(m, backward=False)
        ref = _model(sc, dev, rows=keep.cpu().numpy())
        c2, d2, a2, r2 = render(ref, backward=False)
    finally:
        G.set_near_far_thread(prev)
    assert torch.equal(c1, c2) and torch.equal(d1, d2) and torch.equal(a1, a2) and torch.equal(r1, r2)
    assert not torch.equal(c0, c1)                                            # the prune DID change pixels:
    tx, ty = NF.ROW_TILES[bad]                                                # those of the row's tile, and only those
    moved = (c0 != c1).any(0)
    assert float(moved[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].float().mean()) > 0.9
