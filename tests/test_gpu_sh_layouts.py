"""GPU tests of the rasterizer on every legal (SH degree, coefficient count) pair and on misaligned caller tensors
(tests/sh_layouts.py; the CPU side is tests/test_sh_layouts.py).

The C ABI takes the active degree D and the coefficients per Gaussian M separately; the rest of the suite runs the four
pairs M = (D+1)^2.  Here: all 38 pairs against float64 and against the oracle; every output element written, the
gradient of the coefficients beyond the active degree exactly zero; the product forward equal to the debug forward bit for
bit, also where a workgroup walks several blocks (200 003 Gaussians); and every caller tensor at 4 / 8 / 12 bytes inside
guarded allocations, bit-identical to the aligned run.  Every case asserts the launch cell it is there for
(sh_layouts.launch_cells, computed from the pointers actually handed in)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import depth_ref as DR
import gs_livm_amd as G
import ref64 as R
import sh_layouts as L
from arena import PAT, Arena
from gs_livm_amd import _capi
from gs_livm_amd import synthetic as S
from helpers import GRAD_NAMES, grad_close, hip_backward, hip_forward
from oracle import oracle as O
from test_gpu_parity import MODES, check_forward, masked_grads, oracle_forward
from test_gpu_ref64 import SAMPLE, _hip_vs_f64

pytestmark = pytest.mark.gpu
SCENE_IDS = {L.SMALL: "P300", L.MID: "P1500"}
PAIR_CASES = [(L.SMALL, D, M) for D, M in L.PAIRS] + [(L.MID, D, M) for D, M in L.VARIANT_PAIRS]
PAIR_IDS = ["%s-D%d-M%d" % (SCENE_IDS[s], D, M) for s, D, M in PAIR_CASES]


def _cells(P, D, M, debug, t=None, **kw):
    """The launch cell from the pointers of the tensors handed in (allocator tensors: 16-byte aligned)."""
    if t is not None:
        kw.setdefault("shs_ptr", t["shs"].data_ptr())
    return L.launch_cells(P, D, M, debug, **kw)


def _expected_forward(M, D, debug):
    """What an aligned, plain-input forward must run, stated apart from launch_cells: M = 1 is not staged, the
    pipelined variants take M = 4 and 16 unless the debug copy of cov3D is wanted, the block copy the rest."""
    if M == 1:
        return "general" if debug else "plain"
    if debug or M not in (4, 16):
        return "block_copy"
    return "rowk12" if M == 16 else "rowk3"


# ---- 1. every pair against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,D,M", PAIR_CASES, ids=PAIR_IDS)
def test_every_pair_against_f64(scene, D, M, gpu_device):
    """Both binning modes x debug and product passes, images and the nine gradient groups, at the unchanged bars
    (helpers.check_against_ref64).  At 1 500 the last block has 220 Gaussians: its partial block spans all four waves."""
    P, W, H, seed = scene
    worst = _hip_vs_f64(L.with_layout(P, W, H, seed, D, M), seed, gpu_device)
    print("HIP (D, M) = (%d, %d) on %r: worst |d| / bar %.3f" % (D, M, scene, max(worst.values())))
    assert max(worst.values()) < 1.0


# ---- 2. every pair against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,D,M", PAIR_CASES, ids=PAIR_IDS)
def test_every_pair_against_the_oracle(scene, D, M, gpu_device):
    """check_forward in both modes, debug and product: the exact stages bit for bit, colours from SH within 1e-6, clamp
    flags exact; the gradients with grad_close; the gradient of the unused coefficients and of culled rows exactly 0."""
    P, W, H, seed = scene
    sc = L.with_layout(P, W, H, seed, D, M)
    O.set_threads(min(O.max_threads(), 16))
    used = (D + 1) ** 2
    for mode in MODES:
        fr = oracle_forward(sc, mode)
        dcol, dacc = masked_grads(W, H, seed, fr.fragile)
        ref = O.backward(fr, sc, dcol, dacc)
        assert not ref["dL_dsh"].reshape(P, M, 3)[:, used:].any()
        for debug in (True, False):
            t, fwd = hip_forward(sc, gpu_device, debug=debug, ref_rects=(mode == "reference"))
            assert t["shs"].data_ptr() % 16 == 0
            assert _cells(P, D, M, debug, t)["forward"] == _expected_forward(M, D, debug)
            check_forward(sc, fr, fwd, gpu_device, debug=debug)
            got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device, debug=debug)
            for k in GRAD_NAMES:
                grad_close(got[k], ref[k], k)
                assert not got[k].reshape(P, -1)[fr.radii <= 0].any(), k
            assert not got["dL_dsh"][:, used:].any()
            assert got["dL_dsh"][:, :used].any()


# ---- the C ABI called directly on Arena views (items 3 and 5) --------------------------------------------------------
INPUTS = ("means3D", "scales", "rotations", "opacities", "shs", "colors_precomp", "cov3D_precomp", "viewmatrix",
          "projmatrix", "campos", "bg")
IMAGES = ("out_color", "out_depth", "out_acc")
GRADS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations")   # gsr_backward's order of outputs


def _abi_frame(sc, up, dev, off_of, depth=True, debug=False):
    """One forward and one backward through the C ABI itself, every caller tensor a view of an Arena (inputs copied in,
    outputs prefilled with PAT).  up = (dL_dpix, dL_dacc, dL_ddepth).  Returns (arena, num_rendered)."""
    a = Arena(dev, off_of)
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    M = 0 if sc.get("shs") is None else sc["shs"].shape[1]
    for k in INPUTS:
        if sc.get(k) is not None:
            a.put(k, torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev))
    a.put("out_color", shape=(3, H, W)), a.put("out_depth", shape=(1, H, W)), a.put("out_acc", shape=(1, H, W))
    radii = a.put("radii", shape=(P,)).view(torch.int32)
    for k, g in zip(("dL_dpix", "dL_dacc", "dL_ddepth"), up):
        a.put(k, torch.from_numpy(np.ascontiguousarray(g)).to(dev))
    shapes = dict(dL_dmeans2D=(P, 3), dL_dconic=(P, 2, 2), dL_dopacity=(P, 1), dL_dcolors=(P, 3), dL_dmeans3D=(P, 3),
                  dL_dcov3D=(P, 6), dL_dsh=(P, M, 3), dL_dscales=(P, 3), dL_drotations=(P, 4), dL_ddepths=(P,))
    for k in GRADS + ("dL_ddepths",):
        a.put(k, shape=shapes[k])
    p = lambda k: C.c_void_p(a.ptr(k)) if k in a.t and a.t[k].numel() else None  # noqa: E731
    lib = G.lib()
    gb, bb, ib = _capi._Blob(dev), _capi._Blob(dev), _capi._Blob(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    D, mod = int(sc["sh_degree"]), float(sc.get("scale_modifier", 1.0))
    prev, prev_nf = G.set_reference_rects_thread(False), G.set_near_far_thread(False)
    try:
        key = lib.gsr_forward(gb.fn, None, bb.fn, None, ib.fn, None, P, D, M, p("bg"), W, H, p("means3D"), p("shs"),
                              p("colors_precomp"), p("opacities"), p("scales"), mod, p("rotations"), p("cov3D_precomp"),
                              p("viewmatrix"), p("projmatrix"), p("campos"), float(sc["tanfovx"]), float(sc["tanfovy"]),
                              0, p("out_color"), p("out_depth"), p("out_acc"), C.c_void_p(radii.data_ptr()),
                              int(debug), stream)
    finally:
        G.set_reference_rects_thread(prev)
        G.set_near_far_thread(prev_nf)
    assert key >= 0, lib.gsr_last_error()
    blobs = [C.c_void_p(b.tensor.data_ptr()) if b.tensor.numel() else C.c_void_p(1) for b in (gb, bb, ib)]
    common = (P, D, M, key, p("bg"), W, H, p("means3D"), p("shs"), p("colors_precomp"), p("scales"), mod, p("rotations"),
              p("cov3D_precomp"), p("viewmatrix"), p("projmatrix"), p("campos"), float(sc["tanfovx"]),
              float(sc["tanfovy"]), C.c_void_p(radii.data_ptr()), *blobs, p("dL_dpix"), p("dL_dacc"))
    outs = [p(k) for k in GRADS]
    if depth:
        rc = lib.gsr_backward_depth(*common, p("dL_ddepth"), *outs, p("dL_ddepths"), int(debug), stream)
    else:
        rc = lib.gsr_backward(*common, *outs, int(debug), stream)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    a.keep = (gb, bb, ib)
    return a, G.last_num_rendered()


def _outputs(a, depth=True):
    names = IMAGES + ("radii",) + GRADS + (("dL_ddepths",) if depth else ())
    return {k: a.t[k].view(torch.int32).clone() for k in names}       # bit patterns


def _no_pattern_left(a, depth=True):
    for k, v in _outputs(a, depth).items():
        assert not bool((v == PAT).any()), "%s: an element was not written" % k
    assert a.guards_intact() is None, a.guards_intact()


def _zero_rows(a, sc, D, M, depth=True):
    P = sc["means3D"].shape[0]
    hidden = a.t["radii"].view(torch.int32) <= 0
    assert 0 < int(hidden.sum()) < P
    for k in GRADS + (("dL_ddepths",) if depth else ()):
        if a.t[k].numel():
            assert not bool(a.t[k].reshape(P, -1)[hidden].any()), k
    if M:
        used = (D + 1) ** 2
        assert not bool(a.t["dL_dsh"][:, used:].any())              # on every row, visible or not
        assert bool(a.t["dL_dsh"][:, :used].any())


@functools.lru_cache(maxsize=None)
def _depth_reference(scene, D, M):
    P, W, H, seed = scene
    sc = L.with_layout(P, W, H, seed, D, M)
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc)
    up = DR.upstream(sc, fr, seed, "all")
    return sc, fr, up


# ---- 3. every output element is written ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", L.VARIANT_PAIRS)
def test_every_output_element_is_written(D, M, gpu_device):
    """gsr_backward into outputs prefilled with a NaN pattern (the Python host allocates with torch.empty because "the
    library overwrites every element"): no pattern left, the coefficients beyond the active degree and the rows of
    culled Gaussians exactly zero."""
    sc, fr, up = _depth_reference(L.MID, D, M)
    a, _ = _abi_frame(sc, up, gpu_device, lambda name, i: 0, depth=False)
    assert L.launch_cells(sc["means3D"].shape[0], D, M, False, a.ptr("shs"), a.ptr("dL_dsh"))["backward"] == "staged"
    _no_pattern_left(a, depth=False)
    assert bool((a.t["dL_ddepths"].view(torch.int32) == PAT).all())    # gsr_backward does not know this output
    _zero_rows(a, sc, D, M, depth=False)


@pytest.mark.parametrize("D,M", L.DEPTH_PAIRS)
def test_every_output_element_is_written_depth(D, M, gpu_device):
    """The same through gsr_backward_depth, held to depth_ref.render64 at test_gpu_depth_grad.py's bar."""
    sc, fr, up = _depth_reference(L.SMALL, D, M)
    P = sc["means3D"].shape[0]
    a, _ = _abi_frame(sc, up, gpu_device, lambda name, i: 0, depth=True)
    cells = L.launch_cells(P, D, M, False, a.ptr("shs"), a.ptr("dL_dsh"), depth=True)
    assert cells["backward"] == ("unstaged+depth" if M == 1 else "staged+depth")
    _no_pattern_left(a)
    _zero_rows(a, sc, D, M)
    r = DR.render64(sc, fr, *up, slack=True)
    got = {k: a.t[k].cpu().numpy() for k in GRADS + ("dL_ddepths",)}
    for k in GRAD_NAMES + ("dL_ddepths",):
        ref = r[k].reshape(got[k].shape)
        grad_close(got[k], ref, k, slack=r["slack"][k])
    worst = DR.ratios(got, r, GRAD_NAMES + ("dL_ddepths",))
    print("depth backward (D, M) = (%d, %d): worst |d| / bar %.3f" % (D, M, max(worst.values())))
    assert np.abs(got["dL_ddepths"]).max() > 0


# ---- 4. product forward = debug forward, bit for bit -----------------------------------------------------------------
def _product_equals_debug(sc, dev):
    t, dbg = hip_forward(sc, dev, debug=True)
    G.set_binning_capacity_hint(0)
    t2, prod = hip_forward(sc, dev, debug=False)                  # synchronous
    t3, again = hip_forward(sc, dev, debug=False)                 # speculative
    assert int(dbg[0]) == int(prod[0]) == int(again[0]) > 0       # instance count
    for i in (1, 2, 3, 4):                                        # colour, depth, silhouette, radii
        assert torch.equal(dbg[i], prod[i]) and torch.equal(dbg[i], again[i]), i
    return t3, again


@pytest.mark.parametrize("D,M", L.VARIANT_PAIRS)
def test_product_forward_equals_debug_forward(D, M, gpu_device):
    P, W, H, seed = L.MID
    sc = L.with_layout(P, W, H, seed, D, M)
    t, fwd = _product_equals_debug(sc, gpu_device)
    assert _cells(P, D, M, False, t)["forward"] == _expected_forward(M, D, False)
    assert _cells(P, D, M, True, t)["forward"] == "block_copy"


@pytest.mark.parametrize("D,M", L.SCALE_PAIRS)
def test_product_forward_equals_debug_forward_at_scale(D, M, gpu_device):
    """200 003 Gaussians = 782 blocks on 391 workgroups: every workgroup walks two blocks, so the pipelined variants
    fetch a next block's rows (they do not below 196 608 Gaussians), the last block partial.  The per-Gaussian backward
    against ref64.gaussian_vjp on a 4 096 sample, as test_gpu_ref64.test_per_gaussian_stage_at_scale."""
    P, W, H, seed = L.LARGE
    sc = L.with_layout(P, W, H, seed, D, M)
    t, fwd = _product_equals_debug(sc, gpu_device)
    assert P > 3 * 256 * 256 and _cells(P, D, M, False, t)["forward"] == _expected_forward(M, D, False)
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device, debug=False)
    used = (D + 1) ** 2
    assert not got["dL_dsh"][:, used:].any() and got["dL_dsh"][:, :used].any()
    radii = fwd[4].cpu().numpy()
    two_d = np.concatenate([np.abs(got[k]).reshape(P, -1) for k in
                            ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors")], 1).max(1) > 0
    assert not two_d[radii <= 0].any()
    cand = np.flatnonzero(two_d)
    assert cand.size >= 1000
    idx = np.sort(np.random.default_rng(seed).choice(cand, size=min(SAMPLE, cand.size), replace=False))
    v = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], W, H)
    cl = v["clamped"].cpu().numpy()
    clamped = np.stack([(cl >> k) & 1 for k in range(3)], 1).astype(bool)
    g3 = R.gaussian_vjp(sc, idx, clamped, R.upstream_from_reference_arrays(got, idx))
    ref = {"dL_dmeans3D": g3["means3D"].numpy(), "dL_dcov3D": g3["cov6"].numpy(), "dL_dsh": g3["shs"].numpy(),
           "dL_dscales": g3["scales"].numpy(), "dL_drotations": g3["rotations"].numpy()}
    for k, want in ref.items():
        grad_close(got[k][idx], want, k)
    assert (np.abs(got["dL_dmeans3D"][idx]).max(1) > 0).all()


# ---- 5. alignment -----------------------------------------------------------------------------------------------------
def _align_scene(kind, D, M):
    sc, fr, up = _depth_reference(L.SMALL, D, M)
    sc = dict(sc)
    if kind == "colors_precomp":
        sc["colors_precomp"] = np.random.default_rng(5).uniform(0, 1, (L.SMALL[0], 3)).astype(np.float32)
        sc["shs"] = None
    elif kind == "cov3D_precomp":
        cov = fr.cov3D.copy()
        cov[fr.radii <= 0] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32)
        sc["cov3D_precomp"], sc["scales"], sc["rotations"] = cov, None, None
    return sc, up


def _check_placements(sc, up, D, M, modes, dev, **cell_kw):
    P = sc["means3D"].shape[0]
    base, R0 = _abi_frame(sc, up, dev, lambda name, i: 0)
    _no_pattern_left(base)
    want = _outputs(base)
    for mode in modes:
        off_of = L.placement(mode)
        a, R1 = _abi_frame(sc, up, dev, off_of)
        for k, t in a.t.items():                                   # the placement is the one that was asked for
            assert t.numel() == 0 or t.data_ptr() % 16 == off_of(k), (mode, k)
        assert "rotations" not in a.t or a.ptr("rotations") % 16 == 0          # the contract (include/gsraster.h)
        shs_ptr = (a.ptr("shs") or 0) if "shs" in a.t else 0       # (absent with precomputed colours)
        dsh_ptr = a.ptr("dL_dsh") or 0
        cells = L.launch_cells(P, D, M, False, shs_ptr, dsh_ptr, depth=True, **cell_kw)
        assert cells == L.launch_cells(P, D, M, False, L.placed_offset(mode, "shs"), L.placed_offset(mode, "dL_dsh"),
                                       depth=True, **cell_kw), mode     # the cell tests/test_sh_layouts.py counted
        if M in (4, 16) and not cell_kw:   # the pipelined variants need 16-byte rows: the block copy takes the rest
            assert cells["forward"] == (("rowk12" if M == 16 else "rowk3") if shs_ptr % 16 == 0 else "block_copy"), mode
            assert cells["shs_full"] == (("vec16" if shs_ptr % 16 == 0 else "scalar"), "0mod4")
        if M > 1:
            assert cells["dL_dsh"][0] == ("vec16" if (3 * M) % 4 == 0 and dsh_ptr % 16 == 0 else "scalar"), mode
        assert R1 == R0
        _no_pattern_left(a)
        got = _outputs(a)
        for k in want:                                             # only copies differ between the two runs
            assert torch.equal(got[k], want[k]), (mode, k)
        b, _ = _abi_frame(sc, up, dev, off_of)                     # two runs are bit-equal
        again = _outputs(b)
        for k in want:
            assert torch.equal(again[k], got[k]), (mode, k, "second run")
        assert b.guards_intact() is None


@pytest.mark.parametrize("D,M", L.ALIGN_PAIRS)
def test_misaligned_caller_tensors(D, M, gpu_device):
    """Every input and output of gsr_forward and gsr_backward_depth at 4 / 8 / 12 bytes inside guarded allocations
    (`rotations` 16-byte aligned inside its guard: the contract): bit-identical to the same build's all-aligned run,
    which items 1 and 2 hold to float64 and the oracle; guards intact, no output element left unwritten."""
    sc, up = _align_scene("plain", D, M)
    _check_placements(sc, up, D, M, L.PLACEMENTS, gpu_device)


@pytest.mark.parametrize("kind,D,M", [("colors_precomp", 0, 1), ("cov3D_precomp", 1, 8)])
def test_misaligned_precomputed_inputs(kind, D, M, gpu_device):
    sc, up = _align_scene(kind, D, M)
    _check_placements(sc, up, D, M, ("a4", "a8", "a12", "mix") if kind == "colors_precomp" else ("mix",), gpu_device,
                      **{kind: True})


def test_illegal_pair_and_misaligned_rotations_are_refused_on_the_device_too(gpu_device):
    """(1, 2) is no legal pair, and a `rotations` at 4 bytes is refused by the C ABI before anything is enqueued: the
    outputs keep their pattern."""
    sc, up = _align_scene("plain", 0, 2)
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu_device) for k in INPUTS if sc.get(k) is not None}
    buf = torch.zeros(4 * P + 8, device=gpu_device)
    rot4 = buf[1:1 + 4 * P].view(P, 4)
    rot4.copy_(t["rotations"])
    assert rot4.data_ptr() % 16 == 4
    out = torch.full((5 * W * H + P,), PAT, dtype=torch.int32, device=gpu_device)
    o = [C.c_void_p(out.data_ptr() + 4 * n) for n in (0, 3 * W * H, 4 * W * H, 5 * W * H)]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    blob = _capi._Blob(gpu_device)
    lib = G.lib()
    for D, M, rot, code, word in ((L.REFUSED_ALIGN_PAIR[0], L.REFUSED_ALIGN_PAIR[1], t["rotations"], -4, b"SH degree"),
                                  (0, 2, rot4, -1, b"rotations")):
        rc = lib.gsr_forward(blob.fn, None, blob.fn, None, blob.fn, None, P, D, M, p(t["bg"]), W, H, p(t["means3D"]),
                             p(t["shs"]), None, p(t["opacities"]), p(t["scales"]), 1.0, p(rot), None,
                             p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]), float(sc["tanfovx"]),
                             float(sc["tanfovy"]), 0, o[0], o[1], o[2], o[3], 0,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == code and word in lib.gsr_last_error()
    torch.cuda.synchronize()
    assert bool((out == PAT).all())


def _leaves(sc, dev, rot_offset):
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev).requires_grad_(True)
         for k in ("means3D", "opacities", "scales", "shs")}
    P = sc["means3D"].shape[0]
    buf = torch.zeros(4 * P + 8, device=dev)
    n = rot_offset // 4
    with torch.no_grad():
        buf[n:n + 4 * P].copy_(torch.from_numpy(sc["rotations"]).to(dev).reshape(-1))
    t["rotations"] = buf[n:n + 4 * P].view(P, 4).requires_grad_(True)   # a leaf that is a view into a larger buffer
    assert t["rotations"].data_ptr() % 16 == rot_offset and t["rotations"].is_contiguous()
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    return t


@pytest.mark.parametrize("host", ["python", "libtorch"])
def test_operator_surfaces_accept_a_misaligned_rotations(host, gpu_device):
    """A 4-byte-offset `rotations` (what multiview.GaussianBuffer hands out at float offset P (6 + 3M)) through the
    Python and the LibTorch operator surfaces: rendered, and differentiated, bit-identically to the aligned tensor."""
    from test_gpu_depth_grad import _settings
    P, W, H, seed = L.SMALL
    sc = L.with_layout(P, W, H, seed, 1, 8)
    if host == "python":
        from gs_livm_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
        rast = GaussianRasterizer(_settings(GaussianRasterizationSettings, sc, gpu_device))
        call = rast
    else:
        ops = G.torch_ops()
        call = ops.GaussianRasterizer(_settings(ops.GaussianRasterizationSettings, sc, gpu_device)).forward
    res = {}
    for off in (0, 4):
        x = _leaves(sc, gpu_device, off)
        color, radii, depth, acc = call(x["means3D"], x["means2D"], x["opacities"], shs=x["shs"], scales=x["scales"],
                                        rotations=x["rotations"])
        (color.sum() + 0.5 * acc.sum()).backward()
        res[off] = (color.detach(), radii, depth.detach(), acc.detach()) + tuple(
            x[k].grad for k in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"))
    assert res[0][0].any() and res[0][9].any()
    for i, (u, v) in enumerate(zip(res[0], res[4])):
        assert torch.equal(u, v), i
