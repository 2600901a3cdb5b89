"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
the CPU oracle on the same seeded inputs, against the committed golden vectors, and -- at
BASELINE.json's full sizes -- through size-independent properties.

Tolerances (BASELINE.json north_star): integer / index results bit-exact (radii, tile counts,
offsets, sort keys, sorted Gaussian ids, tile ranges, n_contrib); colour / depth / silhouette <= 1e-4 abs;
gradients |d| <= 1e-5 * max|g| + 1e-4 * |g_row|_inf (f32 summation order differs; SURVEY.md Appendix B;
see helpers.grad_close).

Two binning modes (include/gsraster.h, gsr_set_reference_rects), both tested against the matching oracle frame:
  "reference"  the library emits getRect's full 3-sigma tile square (auxiliary.h:39-46, rasterizer_impl.cu:64-125):
               tiles_touched, num_rendered, keys, point_list, RANGES and n_contrib are compared bit for bit with
               O.forward(sc) -- the reference's own definition -- and with the fw_* fields of the golden fixtures;
  "culled"     the product's default: instances are emitted only where the alpha >= 1/255 footprint box overlaps the
               tile; compared with the oracle's `tight` restatement of that rule (oracle/gsr_oracle.c, tighten_rect;
               tests/test_oracle.py proves on the CPU that it leaves every image and gradient bit-identical).

Fragile pixels: the blend has hard cuts (alpha < 1/255 skip, T < 1e-4 stop).  Where the oracle sees
such a test decided by less than rounding distance (frame.fragile), a different-but-valid rounding
(FMA contraction, hardware exp) may flip it and legitimately move the pixel by up to alpha*T.  Those
pixels (a ~1e-4 fraction) are held to the looser bound FRAGILE_TOL, must stay rare, and are masked
out of the upstream gradient in the backward tests; every other pixel is held to 1e-4 with no
exceptions.
"""
import json
import os

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S
from helpers import check_near_far_against_one_chain as _check_near_far_against_one_chain
from helpers import conic_condition, grad_close, hip_backward, hip_forward, to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMG_TOL = 1e-4
FRAGILE_TOL = 2e-2
GRAD_NAMES = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
              "dL_dscales", "dL_drotations")


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def check_forward(sc, fr, fwd, dev, debug=True, max_fragile=5e-3):
    """Every stage of the forward against an oracle frame (or a golden fixture exposing the same fields)."""
    R, color, depth, acc, radii, geom, binning, img = fwd
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    assert R == fr.R
    v = G.state_views(geom, binning, img, P, R, W, H)
    assert v["num_rendered"] == fr.R
    assert np.array_equal(radii.cpu().numpy(), fr.radii)
    assert np.array_equal(_u32(v["tiles_touched"]), fr.tiles_touched)
    if debug:  # the reference's id-order scan is not used by the product; only a debug forward fills the view
        assert np.array_equal(_u32(v["point_offsets"]), fr.point_offsets)
    vis = fr.radii > 0
    sp = v["splats"].cpu().numpy()
    assert np.array_equal(sp[vis, 0:2], fr.means2D[vis])              # bit-exact: feeds the tile rects
    assert np.array_equal(sp[vis, 9], fr.depths[vis])                 # bit-exact: low 32 bits of the keys
    assert np.array_equal(v["depths"].cpu().numpy()[vis], fr.depths[vis])
    assert np.array_equal(sp[vis][:, 2:5], fr.conic_opacity[vis][:, :3])
    assert np.array_equal(sp[vis, 5], fr.conic_opacity[vis, 3])
    if sc.get("colors_precomp") is None:
        assert np.abs(sp[vis, 6:9] - fr.rgb[vis]).max(initial=0) <= 1e-6
        cl = v["clamped"].cpu().numpy()
        bits = np.stack([(cl >> k) & 1 for k in range(3)], 1)
        assert np.array_equal(bits[vis], fr.clamped[vis])
    if sc.get("cov3D_precomp") is None and debug:  # kept by debug forwards only (the backward recomputes it)
        assert np.array_equal(v["cov3D"].cpu().numpy()[vis], fr.cov3D[vis])
    if R:
        assert np.array_equal(v["keys"].cpu().numpy().view(np.uint64), fr.keys)
        assert np.array_equal(_u32(v["point_list"]), fr.point_list)
    assert np.array_equal(_u32(v["ranges"]), fr.ranges)               # THE bit-exact target of BASELINE
    frag = fr.fragile > 0
    assert frag.mean() < max_fragile
    nc, fT = _u32(v["n_contrib"]), v["final_T"].cpu().numpy()
    assert np.array_equal(nc[~frag], fr.n_contrib[~frag])
    for name, got, ref in (("color", color, fr.out_color), ("depth", depth, fr.out_depth), ("acc", acc, fr.out_acc),
                           ("final_T", v["final_T"][None], fr.final_T[None])):
        err = np.abs(got.cpu().numpy() - ref).max(0)
        scale = max(1.0, float(np.abs(ref).max())) if name == "depth" else 1.0  # depth = sum z*alpha*T, z up to 40 m
        assert err[~frag].max(initial=0) <= IMG_TOL * scale, (name, float(err[~frag].max()))
        assert err[frag].max(initial=0) <= FRAGILE_TOL * scale, (name, "fragile", float(err[frag].max()))
    return v


MODES = ("reference", "culled")


def oracle_forward(sc, mode, **kw):
    return O.forward(sc, tight=(mode == "culled"), **kw)


def masked_grads(W, H, seed, fragile):
    dcol, dacc = S.make_upstream_grads(W, H, seed)
    keep = (fragile == 0).astype(np.float32)
    return dcol * keep[None], dacc * keep[None]


SCENES = [  # P, W, H, seed, D
    (300, 70, 50, 11, 3),
    (1, 64, 64, 2, 0),
    (7, 33, 17, 3, 1),
    (2500, 257, 131, 4, 2),
    (10_000, 640, 480, 1, 0),       # BASELINE C1
    (10_000, 640, 480, 1, 3),
    (40_000, 500, 300, 6, 1),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P,W,H,seed,D", SCENES)
def test_forward_backward_parity(P, W, H, seed, D, mode, gpu_device):
    sc = S.make_scene(P, W, H, seed, sh_degree=D)
    fr = oracle_forward(sc, mode)
    if mode == "culled":  # same radii, images and fragile map as the reference's rectangles, bit for bit
        fr_ref = O.forward(sc)
        for k in ("radii", "out_color", "out_depth", "out_acc", "final_T", "fragile"):
            assert np.array_equal(getattr(fr, k), getattr(fr_ref, k)), k
        assert (fr.tiles_touched <= fr_ref.tiles_touched).all()
    t, fwd = hip_forward(sc, gpu_device, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device)
    dcol, dacc = masked_grads(W, H, seed, fr.fragile)
    O.set_threads(1)
    ref = O.backward(fr, sc, dcol, dacc)
    got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device)
    for k in GRAD_NAMES:
        grad_close(got[k], ref[k], k)
    vis = fr.radii > 0
    for k in GRAD_NAMES:  # culled Gaussians receive exact zeros
        assert not got[k].reshape(P, -1)[~vis].any(), k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["oracle_P300_70x50_D3", "oracle_P2000_160x96_D0"])
def test_against_committed_golden_vectors(name, mode, gpu_device):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    P, W, H, seed, D, R = [int(x) for x in z["meta"]]
    sc = dict(W=W, H=H, tanfovx=float(z["in_tanfov"][0]), tanfovy=float(z["in_tanfov"][1]), sh_degree=D,
              scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None,
              **{k: z["in_" + k] for k in ("means3D", "scales", "rotations", "opacities", "shs", "viewmatrix",
                                           "projmatrix", "campos", "bg")})

    class Fix:
        pass
    fr = Fix()
    fr.R = R
    for k in z.files:
        if k.startswith("fw_"):
            setattr(fr, k[3:], z[k])
    if mode == "culled":  # integer stages with the product's culled tile rectangles (oracle tight mode)
        for k in z.files:
            if k.startswith("tw_"):
                setattr(fr, k[3:], z[k])
        fr.R = int(z["meta_tight"][0])
    t, fwd = hip_forward(sc, gpu_device, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device)
    assert not fr.fragile.any()  # the fixtures were chosen without fragile pixels: full-strength gradients
    got = hip_backward(sc, t, fwd, z["dL_dcolor_in"], z["dL_dacc_in"], gpu_device)
    for k in GRAD_NAMES:
        grad_close(got[k], z["bw_" + k], k)


def test_reference_known_answer_through_hip(gpu_device):
    """SURVEY.md Appendix B single-Gaussian values, this time produced by the HIP kernels."""
    from test_oracle import _single
    ka = json.load(open(os.path.join(GOLDEN, "survey_single_gaussian.json")))
    i, e = ka["input"], ka["expected"]
    sc = _single(i["mean"], i["scale"], i["rotation_rxyz"], W=i["width"], H=i["height"], tanx=i["tanfovx"],
                 tany=i["tanfovy"])
    t, fwd = hip_forward(sc, gpu_device)
    v = G.state_views(fwd[5], fwd[6], fwd[7], 1, fwd[0], 640, 480)
    sp = v["splats"].cpu().numpy()[0]
    assert int(fwd[4][0]) == e["radius"]
    # the reference emits the whole 5 x 5 tile square of the 33 px radius (25 instances); the product's default emits
    # the tiles its alpha >= 1/255 footprint box overlaps (the splat is ~6 x 2.5 px sigma: far fewer)
    assert fwd[0] == O.forward(sc, tight=True).R <= e["tiles"] == O.forward(sc).R
    t2, fwd2 = hip_forward(sc, gpu_device, ref_rects=True)
    v2 = G.state_views(fwd2[5], fwd2[6], fwd2[7], 1, fwd2[0], 640, 480)
    assert fwd2[0] == e["tiles"] == int(v2["tiles_touched"][0])   # the survey's reference-produced tile count
    assert torch.equal(fwd2[1], fwd[1]) and torch.equal(fwd2[3], fwd[3])
    assert np.allclose(sp[0:2], e["xy"], atol=1e-4, rtol=0) and np.allclose(sp[2:5], e["conic"], atol=1e-6, rtol=0)


def _same_frame(a, b, P, W, H, what=""):
    """two forwards of the same scene: bit-identical images, radii and internal state"""
    for i, (x, y) in enumerate(zip(a[1:5], b[1:5])):
        assert torch.equal(x, y), (what, i)
    va, vb = (G.state_views(f[5], f[6], f[7], P, f[0], W, H) for f in (a, b))
    assert va["num_rendered"] == vb["num_rendered"] == int(a[0]) == int(b[0])
    for k in ("ranges", "point_list", "n_contrib", "final_T", "tiles_touched", "quad_last"):
        assert torch.equal(va[k], vb[k]), k


def test_speculative_forward_equals_the_synchronous_one(gpu_device):
    """SURVEY.md section 7 / 8(f) #3 (rasterizer_impl.cu:277): from a host thread's second forward on the binning blob
    is sized from the previous frames' instance counts, all kernels are enqueued without waiting for num_rendered
    (they read it from device memory) and the host never blocks.  Results must not depend on the path taken: exact
    prediction, generous prediction, a capacity of exactly R, R + 1, and -- the overflow path -- capacities below R
    (the binning allocator is then called a second time and the chain re-enqueued)."""
    dev = gpu_device
    P, W, H = 30_000, 400, 240
    sc = S.make_scene(P, W, H, 41, sh_degree=1)
    G.set_binning_capacity_hint(0)                       # forget this thread's history
    t, ref = hip_forward(sc, dev, debug=False)           # -> synchronous forward: key == count
    R = int(ref[0])
    assert ref[0].key == R == O.forward(sc, tight=True).R
    dcol, dacc = S.make_upstream_grads(W, H, 41)
    gref = hip_backward(sc, t, ref, dcol, dacc, dev, debug=False)
    before = G.speculation_stats()
    t2, spec = hip_forward(sc, dev, debug=False)         # predicted from the previous frame
    assert spec[0].key > R and int(spec[0]) == R
    _same_frame(ref, spec, P, W, H)
    st = G.speculation_stats()
    assert st["speculative_forwards"] == before["speculative_forwards"] + 1 and st["overflows"] == before["overflows"]
    g2 = hip_backward(sc, t2, spec, dcol, dacc, dev, debug=False)
    for k in gref:
        assert np.array_equal(gref[k], g2[k]), k
    for cap, overflow in ((R, 0), (R + 1, 0), (10 * R, 0), (R - 1, 1), (R // 2, 1), (1000, 1), (1, 1)):
        before = G.speculation_stats()
        G.set_binning_capacity_hint(cap)
        t3, f3 = hip_forward(sc, dev, debug=False)
        st = G.speculation_stats()
        assert st["overflows"] - before["overflows"] == overflow, cap
        assert f3[0].key == (R if overflow else cap) and int(f3[0]) == R
        _same_frame(ref, f3, P, W, H, cap)
        g3 = hip_backward(sc, t3, f3, dcol, dacc, dev, debug=False)
        for k in gref:
            assert np.array_equal(gref[k], g3[k]), (cap, k)
    # a smaller frame after a larger one (capacity far above the count), then an empty one, then a large one again
    small = S.make_scene(500, W, H, 42, sh_degree=1)
    ts, fs = hip_forward(small, dev, debug=False)
    assert int(fs[0]) == O.forward(small, tight=True).R and fs[0].key > int(fs[0])
    none = S.make_scene(500, W, H, 42, sh_degree=1)
    none["means3D"][:, 2] = -1.0
    tn, fn = hip_forward(none, dev, debug=False)
    assert int(fn[0]) == 0 and torch.equal(fn[1], torch.ones_like(fn[1]))
    t4, f4 = hip_forward(sc, dev, debug=False)
    _same_frame(ref, f4, P, W, H)


def test_internal_radii_when_the_caller_passes_none(gpu_device):
    """rasterizer_impl.cu:217-219, 386-388: radii == nullptr -> the geometry state's own array is filled and the
    backward uses it."""
    sc = S.make_scene(3000, 160, 96, 21, sh_degree=1)
    fr = O.forward(sc, tight=True)
    t = to_dev(sc, gpu_device)
    fwd = G.rasterize_forward(t["bg"], t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0,
                              t["cov3D_precomp"], t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], 96, 160,
                              t["shs"], 1, t["campos"], False, True, radii_out=False)
    v = G.state_views(fwd[5], fwd[6], fwd[7], 3000, fwd[0], 160, 96)
    assert np.array_equal(v["radii"].cpu().numpy(), fr.radii)
    dcol, dacc = masked_grads(160, 96, 21, fr.fragile)
    O.set_threads(1)
    ref = O.backward(fr, sc, dcol, dacc)
    g = G.rasterize_backward(t["bg"], t["means3D"], None, t["colors_precomp"], t["scales"], t["rotations"], 1.0,
                             t["cov3D_precomp"], t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"],
                             torch.from_numpy(dcol).to(gpu_device), torch.from_numpy(dacc).to(gpu_device), t["shs"], 1,
                             t["campos"], fwd[5], fwd[0], fwd[6], fwd[7], True)
    grad_close(g[3].cpu().numpy(), ref["dL_dmeans3D"], "dL_dmeans3D")
    grad_close(g[6].cpu().numpy(), ref["dL_dscales"], "dL_dscales")


def test_near_far_frames_equal_one_chain_frames(gpu_device):
    """Near/far binning (gsr_set_near_far, api.hip): budgets from "far below what the pixels need" (most tiles stay
    live: the far chain does nearly all the work) to "more than enough" (the far chain is empty), the redo path when
    the far capacity was predicted too small, and BASELINE C3 itself with the default budget."""
    dev = gpu_device
    try:
        sc = S.make_scene(40_000, 500, 300, 6, sh_degree=1)
        for near_entries in (1, 8, 40, 200):
            st = _check_near_far_against_one_chain(sc, dev, near_entries)
            assert st["near"] + st["far"] <= st["one"]
        assert st["live_tiles"] == st["tiles"]                      # (a sparse scene: no tile ever saturates)
        # a few huge near splats over many small ones: long lists, early saturation in the image centre only
        sc = S.make_scene(60_000, 640, 400, 16, sh_degree=0)
        sc["means3D"][:40, 2] = 1.0
        sc["means3D"][:40, :2] *= 0.3
        sc["scales"][:40] = 0.29
        sc["opacities"][:40] = 0.95
        for near_entries in (4, 64):
            st = _check_near_far_against_one_chain(sc, dev, near_entries)
        assert 0 < st["live_tiles"] < st["tiles"] and st["full_tiles"] < st["tiles"]   # finished centre, live border
        _check_near_far_against_one_chain(sc, dev, 4, far_capacity=100, expect_redo=True)   # far count > capacity
        _check_near_far_against_one_chain(sc, dev, 4)                                        # and afterwards it works
        # far-chain speculation (gsr_set_far_speculation) that turns out wrong: tiles stay live, the far chain is
        # enqueued after the host has seen the count -- same frame, and the backward sorts its tiles itself
        st = _check_near_far_against_one_chain(sc, dev, 4, speculate_far=True)
        assert st["live_tiles"] > 0 and st["far"] > 0 and not st["far_skipped"]
        _check_near_far_against_one_chain(sc, dev, 4, speculate_far=True, far_capacity=100, expect_redo=True)
        # ... and right: a stack of opaque screen-filling splats in front finishes every tile within the near budget
        sc = S.make_scene(30_000, 320, 208, 23, sh_degree=0)
        sc["means3D"][:64, :2] = 0.0
        sc["means3D"][:64, 2] = np.linspace(0.5, 0.9, 64, dtype=np.float32)
        sc["scales"][:64] = 0.29
        sc["opacities"][:64] = 0.98
        st = _check_near_far_against_one_chain(sc, dev, 200, speculate_far=True)
        assert st["live_tiles"] == 0 and st["far"] == 0 and st["far_skipped"]
        # automatic: after two split frames without a live tile the third one speculates
        G.set_far_speculation(None)
        for k in range(3):
            st = _check_near_far_against_one_chain(sc, dev, 200)
            assert st["far_skipped"] == (k == 2), k
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)
    st = G.speculation_stats()
    if os.environ.get("GSR_ASYNC_FAR", "1") != "0":   # stream-side waits exist on MI355X: the speculation ran on two streams
        assert st["async_far_frames"] >= 4, st


@pytest.mark.parametrize("env", [dict(GSR_ASYNC_FAR="0"), dict(GSR_PRE_HIST_MIN_P="0"),
                                 dict(GSR_ASYNC_FAR="0", GSR_PRE_HIST_MIN_P="0"),
                                 dict(GSR_PRE_HIST_MIN_P="0", GSR_FULL_DEPTH_SORT="1")],
                         ids=["host-decided", "partial-sort", "host-decided+partial-sort", "full-depth-sort"])
def test_far_speculation_variants(env, gpu_device):
    """The same hit / miss / redo / automatic cases as above through the other paths of the far-chain speculation, each
    chosen by a knob that is read once per process (child process):
    GSR_ASYNC_FAR=0 -- without stream-side waits the near blend's count of unfinished quads goes to the host mailbox and
    the host enqueues the far chain only if it is non-zero;
    GSR_PRE_HIST_MIN_P=0 -- k_preprocess counts the depth keys' digits on these small scenes too (as it does from 128 k
    Gaussians), so the frames that expect an idle far chain take the PARTIAL depth sort: near candidates compacted and
    sorted on their own, the full sort left to the far chain -- which runs it in the miss cases here;
    GSR_FULL_DEPTH_SORT=1 -- with those counted histograms at hand (GSR_PRE_HIST_MIN_P=0 again: without them there is
    no partial depth sort to switch off) every frame still sorts all Gaussians by depth up front."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import os, sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch, gs_livm_amd as G\nimport test_gpu_parity as T\n"
            "T.test_near_far_frames_equal_one_chain_frames(torch.device('cuda:0'))\n"
            "s = G.speculation_stats()\n"
            "assert s['far_skips'] > 0 and s['far_skip_misses'] > 0, s\n"
            "assert (s['async_far_frames'] == 0) == (os.environ.get('GSR_ASYNC_FAR') == '0'), s\n"
            "print('variant ok')\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "variant ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_two_host_threads_render_concurrently(gpu_device):
    """The reference calls the rasterizer from several host threads.  Two threads, each on a stream of
    its own, render and differentiate a dense scene eight times at the same moment, every frame split near/far with
    far-chain speculation forced: one thread gets the asynchronous mechanism (one per process), the other decides on
    the host; per-thread state (mailbox, counters, histogram pair, predictions) must not mix.  Every frame of both
    threads equals, bit for bit, the frame the main thread rendered alone."""
    import threading
    dev = gpu_device
    sc = S.make_scene(30_000, 320, 208, 23, sh_degree=0)
    sc["means3D"][:64, :2] = 0.0
    sc["means3D"][:64, 2] = np.linspace(0.5, 0.9, 64, dtype=np.float32)
    sc["scales"][:64] = 0.29
    sc["opacities"][:64] = 0.98
    dcol, dacc = S.make_upstream_grads(sc["W"], sc["H"], 5)
    G.set_binning_capacity_hint(0)
    t0, one = hip_forward(sc, dev, debug=False)                     # the reference frame: synchronous, one chain
    g_ref = hip_backward(sc, t0, one, dcol, dacc, dev, debug=False)
    torch.cuda.synchronize()
    errors, skipped = [], []
    t_in = to_dev(sc, dev)

    def forward():  # hip_forward sets the binning mode and near/far for the CALLING THREAD only (gsr_set_*_thread)
        return hip_forward(sc, dev, debug=False, near_far=True)[1]

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                G.set_binning_capacity_hint(0)
                forward()                                           # this thread's first forward is synchronous
                for it in range(8):
                    G.set_near_far_hints(200, None)
                    G.set_far_speculation(True)
                    t, fwd = t_in, forward()
                    g = hip_backward(sc, t, fwd, dcol, dacc, dev, debug=False)
                    for i, (x, y) in enumerate(zip(one[1:5], fwd[1:5])):
                        assert torch.equal(x, y), (k, it, i)
                    for name in g_ref:
                        assert np.array_equal(g_ref[name], g[name]), (k, it, name)
                    stream.synchronize()
                    skipped.append(G.last_far_skipped())
                G.set_near_far_hints(None, None)
                G.set_far_speculation(None)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    # the PROCESS-WIDE switches say the opposite of what the workers need: per-thread settings must win
    prev_nf, prev_rr = G.set_near_far(False), G.set_reference_rects(True)
    try:
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
    finally:
        G.set_near_far(prev_nf)
        G.set_reference_rects(prev_rr)
    assert not any(th.is_alive() for th in threads), "a rendering thread hangs"
    assert not errors, errors
    assert len(skipped) == 16 and all(skipped)                      # every frame completed without a far chain


def test_c3_near_far(c3, gpu_device):
    """BASELINE C3 binned near/far with the default budget (the configuration bench.py times): bit-identical images,
    n_contrib and gradients; every tile is finished by the near phase and the far chain has nothing left to emit."""
    sc, t, fwd = c3
    st = _check_near_far_against_one_chain(sc, gpu_device, None)
    assert st["live_tiles"] == 0 and st["far"] == 0 and st["near"] < st["one"] // 4
    try:  # and without a far chain at all (far-chain speculation, the steady state of bench.py)
        st = _check_near_far_against_one_chain(sc, gpu_device, None, speculate_far=True)
        assert st["far_skipped"] and st["far"] == 0
    finally:
        G.set_far_speculation(None)


def test_c2_near_far(gpu_device):
    """BASELINE C2 (500 k Gaussians, 1280x720: 3.1 near budgets of instances) is a near/far frame by the library's own
    rule -- no hook sets the budget -- and bit-identical to its one-chain frame; the near chain bins a third of it."""
    P, W, H, seed = S.CONFIGS["C2"]
    sc = S.make_scene(P, W, H, seed)
    st = _check_near_far_against_one_chain(sc, gpu_device, None)
    assert st["live_tiles"] == 0 and st["far"] == 0 and st["near"] < st["one"] // 2


def _stack_scene(P=30_000, W=320, H=208, seed=23):
    """Dense where it matters: a stack of 64 opaque splats in front of the camera at yaw 0 finishes every tile they
    cover inside a small near budget; seen from other yaws the stack leaves part of the image, whose tiles stay live."""
    g = S.make_gaussians(P, seed, sh_degree=0, aspect=W / H)
    g["means3D"][:64, :2] = 0.0
    g["means3D"][:64, 2] = np.linspace(0.5, 0.9, 64, dtype=np.float32)
    g["scales"][:64] = 0.29
    g["opacities"][:64] = 0.98
    return g


@pytest.mark.parametrize("n_views", [3, 20])
def test_several_split_forwards_outstanding_then_their_backwards(n_views, gpu_device):
    """The reference's loop (lioOptimization.cpp:1691-1737, 1822-1832): several DIFFERENT views are rendered forward,
    their losses summed, ONE backward.  Here every forward is a split (near/far) frame with far-chain speculation forced
    -- asynchronous where the device has stream-side waits -- and nothing waits between them: n_views frames are
    outstanding, hits (the far chain stays closed) and misses (it runs on the second stream) interleaved, before the
    first backward is enqueued.  Images and every gradient of every view are bit-identical to that view's synchronous
    one-chain frame, which is checked against the oracle.  Twenty views: more frames in flight than the eight outcome
    slots of the mailbox and than the sixteen notes the library used to keep per process -- no backward may lose its
    forward's note (gsr_frame_note_misses), and every outcome is either counted or reported lost."""
    dev = gpu_device
    W, H = 320, 208
    g = _stack_scene(W=W, H=H)
    yaws = np.linspace(-21.0, 21.0, n_views)
    dcol, dacc = S.make_upstream_grads(W, H, 5)
    scenes, ref_img, ref_grad = [], [], []
    G.set_binning_capacity_hint(0)
    O.set_threads(min(O.max_threads(), 8))
    for i, yaw in enumerate(yaws):
        sc = dict(g, **S.make_camera(W, H, yaw_deg=float(yaw)), bg=np.ones(3, np.float32), scale_modifier=1.0,
                  colors_precomp=None, cov3D_precomp=None)
        t, one = hip_forward(sc, dev, debug=False)              # one chain (near/far off for this thread)
        assert not G.last_near_far()[0]
        g1 = hip_backward(sc, t, one, dcol, dacc, dev, debug=False)
        if i % 7 == 0:                                           # ... itself within tolerance of the oracle
            fr = O.forward(sc, tight=True)
            check_forward(sc, fr, one, dev, debug=False)
            dc, da = masked_grads(W, H, 5, fr.fragile)
            want = O.backward(fr, sc, dc, da)
            got = hip_backward(sc, t, one, dc, da, dev, debug=False)
            for k in GRAD_NAMES:
                grad_close(got[k], want[k], k)
        scenes.append(sc)
        ref_img.append([x.clone() for x in one[1:5]])
        ref_grad.append(g1)
    before = G.speculation_stats()
    frames = []
    try:
        for sc in scenes:                                        # n_views forwards, nothing waits in between
            G.set_near_far_hints(24, None)
            G.set_far_speculation(True)
            frames.append(hip_forward(sc, dev, debug=False, near_far=True))
            assert G.last_near_far()[0]
        for sc, (t, fwd), img, g1 in zip(scenes, frames, ref_img, ref_grad):
            g2 = hip_backward(sc, t, fwd, dcol, dacc, dev, debug=False)
            for i, (x, y) in enumerate(zip(img, fwd[1:5])):
                assert torch.equal(x, y), i
            for k in g1:
                assert np.array_equal(g1[k], g2[k]), k
        torch.cuda.synchronize()
        assert G.async_outcomes_pending() == 0                   # everything has arrived by now
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)
    st = G.speculation_stats()
    d = {k: st[k] - before[k] for k in before if k != "near_budget_scale_q8"}
    assert d["near_far_forwards"] == n_views and d["overflows"] == 0 and d["frame_note_misses"] == 0, d
    # every frame's outcome was counted as a hit or a miss, or reported lost (a ninth asynchronous frame in flight)
    assert d["far_skips"] + d["far_skip_misses"] + d["async_outcomes_lost"] == n_views, d
    assert d["far_skips"] > 0 and (d["far_skip_misses"] > 0 or d["async_outcomes_lost"] > 0), d
    if os.environ.get("GSR_ASYNC_FAR", "1") != "0":
        assert d["async_far_frames"] == n_views, d


def test_asynchronous_miss_frame_at_1080p_without_partial_sort(gpu_device):
    """An asynchronous frame whose near chain leaves most tiles unfinished, at 1920x1080 and with fewer than 128 k
    Gaussians -- no partial depth sort, so the first kernel of the far chain on the second stream (k_live_sat) reads what
    the near blend's 32 640 waves stored (quad_done, parked pixel state) the moment it is released.  The release comes
    from behind the near blend's kernel boundary (k_decide_far): bit-identical to the one-chain frame."""
    sc = S.make_scene(100_000, 1920, 1080, 41, sh_degree=0)
    try:
        for _ in range(3):
            st = _check_near_far_against_one_chain(sc, gpu_device, 12, speculate_far=True)
            assert st["live_tiles"] > st["tiles"] // 2 and st["far"] > 0 and not st["far_skipped"]
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


def test_empty_input_is_a_noop(gpu_device):
    """rasterize_points.cu:92-93,183: P == 0 -> num_rendered 0, zero images, empty grads."""
    sc = S.make_scene(0, 64, 48, 1)
    t, fwd = hip_forward(sc, gpu_device)
    assert fwd[0] == 0 and fwd[4].numel() == 0
    assert not fwd[1].any() and not fwd[2].any() and not fwd[3].any()
    g = hip_backward(sc, t, fwd, *S.make_upstream_grads(64, 48, 1), gpu_device)
    assert all(v.size == 0 for v in g.values())


def test_everything_culled(gpu_device):
    sc = S.make_scene(500, 100, 60, 8)
    sc["means3D"][:, 2] = -2.0
    fr = O.forward(sc, tight=True)
    t, fwd = hip_forward(sc, gpu_device)
    assert fwd[0] == 0 == fr.R
    assert torch.equal(fwd[1], torch.ones_like(fwd[1])) and not fwd[3].any()  # background only
    g = hip_backward(sc, t, fwd, *S.make_upstream_grads(100, 60, 8), gpu_device)
    assert all(not v.any() for v in g.values())


def _variant(P=1500, W=200, H=120, seed=13, D=1):
    return S.make_scene(P, W, H, seed, sh_degree=D)


def _full_check(sc, dev, seed=13, stress=False, mode="culled"):
    fr = oracle_forward(sc, mode)
    t, fwd = hip_forward(sc, dev, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, dev, max_fragile=2e-2 if stress else 5e-3)  # needles widen the uncertainty windows
    dcol, dacc = masked_grads(sc["W"], sc["H"], seed, fr.fragile)
    O.set_threads(1)
    ref = O.backward(fr, sc, dcol, dacc)
    got = hip_backward(sc, t, fwd, dcol, dacc, dev)
    cond = conic_condition(fr.conic_opacity) if stress else None
    for k in GRAD_NAMES:
        grad_close(got[k], ref[k], k, cond=cond)
    return fr, got


@pytest.mark.parametrize("mode", MODES)
def test_precomputed_colors_path(mode, gpu_device):
    sc = _variant()
    rng = np.random.default_rng(1)
    sc["colors_precomp"] = rng.uniform(0, 1, (1500, 3)).astype(np.float32)
    sc["shs"] = None
    fr, got = _full_check(sc, gpu_device, mode=mode)
    assert got["dL_dsh"].size == 0 and np.abs(got["dL_dcolors"]).max() > 0


@pytest.mark.parametrize("mode", MODES)
def test_precomputed_cov3d_path(mode, gpu_device):
    sc = _variant()
    base = O.forward(sc)
    cov = base.cov3D.copy()
    cov[base.radii <= 0] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32)
    sc["cov3D_precomp"] = cov
    sc["scales"] = None
    sc["rotations"] = None
    fr, got = _full_check(sc, gpu_device, mode=mode)
    assert np.abs(got["dL_dcov3D"]).max() > 0 and not got["dL_dscales"].any() and not got["dL_drotations"].any()


@pytest.mark.parametrize("mode", MODES)
def test_scale_modifier_and_black_background(mode, gpu_device):
    sc = _variant(seed=14)
    sc["scale_modifier"] = 0.6
    sc["bg"] = np.array([0.0, 0.25, 0.5], np.float32)
    _full_check(sc, gpu_device, seed=14, mode=mode)


@pytest.mark.parametrize("mode", MODES)
def test_transparent_and_opaque_extremes(mode, gpu_device):
    sc = _variant(P=800, seed=15)
    sc["opacities"][:200] = 0.003   # < 1/255: can never contribute
    sc["opacities"][200:400] = 1.0  # alpha saturates at 0.99
    fr, got = _full_check(sc, gpu_device, seed=15, mode=mode)
    assert not got["dL_dopacity"][:200].any()


@pytest.mark.parametrize("mode", MODES)
def test_screen_filling_splats_and_long_lists(mode, gpu_device):
    """Few huge splats (hundreds of tiles each) over many small ones: long per-tile lists (> 1 chunk of
    256), early termination, and Gaussians whose rect is clamped at all four image borders."""
    sc = S.make_scene(6000, 320, 200, 16, sh_degree=0)
    sc["means3D"][:20, 2] = 1.0
    sc["means3D"][:20, :2] *= 0.2
    sc["scales"][:20] = 0.29
    sc["means3D"][20:, 2] = np.random.default_rng(2).uniform(6.0, 9.0, 5980).astype(np.float32)
    sc["means3D"][20:, :2] = np.random.default_rng(3).uniform(-0.6, 0.6, (5980, 2)).astype(np.float32)
    fr, _ = _full_check(sc, gpu_device, seed=16, mode=mode)
    r = fr.ranges.astype(np.int64)
    assert (r[:, 1] - r[:, 0]).max() > 512 and fr.tiles_touched.max() >= 100


def test_screen_filling_runs_shared_by_the_gather(gpu_device):
    """Gaussians that cover the whole image at 1024 x 768 (3072 tiles): their slot runs are longer than the 2048 slots
    from which k_gather_records shares a run among the four waves of a workgroup (a camera that turns towards a near
    Gaussian sees such splats).  Against the oracle, and one chain (gather over the touched list) against near/far
    (gather over the chains' descriptors) bit for bit."""
    sc = S.make_scene(3000, 1024, 768, 31, sh_degree=0)
    sc["means3D"][:12, 2] = np.linspace(1.0, 1.3, 12, dtype=np.float32)
    sc["means3D"][:12, :2] *= 0.02
    sc["scales"][:12] = 0.3       # (the largest the reference draws: scale x modifier > 0.3 is culled, forward.cu:227-229)
    sc["opacities"][:12] = 0.04   # (thin: every pixel keeps taking splats behind them)
    fr, _ = _full_check(sc, gpu_device, seed=31, mode="culled")
    assert int((fr.tiles_touched > 2048).sum()) >= 12
    st = _check_near_far_against_one_chain(sc, gpu_device, near_entries=6)
    assert st["far"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_depth_ties_keep_id_order(mode, gpu_device):
    """Thousands of Gaussians share each of a few depths: inside a tile the reference's 64-bit keys then tie and its
    stable sort leaves such instances in ascending Gaussian id.  Here that order has to survive
    the depth sort's four look-back passes and the tile sort's LDS-atomic ranking (the production path: ranks from the
    order in which one ds_add_rtn serves the lanes that hit one address) -- lists bit-exact against the oracle, and the
    debug forward's own check of every list (k_verify_sorted_lists) stays silent."""
    sc = S.make_scene(30_000, 400, 300, 31, sh_degree=0)
    z = sc["means3D"][:, 2]
    vis = z > 0.5
    z[vis] = np.float32(1.5) + np.floor(z[vis] / 5.0).astype(np.float32) * np.float32(4.25)   # eight depth levels
    fr = oracle_forward(sc, mode)
    keys = np.unique(fr.depths[fr.radii > 0].view(np.uint32))
    assert keys.size <= 9 and (fr.radii > 0).sum() > 10_000
    t, fwd = hip_forward(sc, gpu_device, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device)


@pytest.mark.parametrize("mode", MODES)
def test_large_image_many_tile_bits(mode, gpu_device):
    """3000x1700: 188 x 107 = 20116 tiles -> 15 tile-id bits (two 8-bit sort passes), rect origins beyond 127,
    partial tiles on both borders."""
    sc = S.make_scene(30_000, 3000, 1700, 18, sh_degree=0)
    O.set_threads(min(O.max_threads(), 16))
    fr = oracle_forward(sc, mode, keep_handle=False)
    t, fwd = hip_forward(sc, gpu_device, debug=False, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device, debug=False)
    assert int(fr.ranges.max()) == fr.R and fr.ranges.shape[0] == 188 * 107


@pytest.mark.parametrize("mode", MODES)
def test_huge_image_32bit_tile_keys(mode, gpu_device):
    """4112 x 4112: 257 x 257 = 66049 tiles > 65536, so the tile sort runs on 32-bit keys (17 tile-id bits, three
    passes) instead of the 16-bit path every other test takes."""
    sc = S.make_scene(20_000, 4112, 4112, 23, sh_degree=0)
    O.set_threads(min(O.max_threads(), 16))
    fr = oracle_forward(sc, mode, keep_handle=False)
    t, fwd = hip_forward(sc, gpu_device, debug=False, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device, debug=False)
    assert fr.ranges.shape[0] == 257 * 257 and int(fr.ranges.max()) == fr.R


@pytest.mark.parametrize("D,P", [(1, 200_003), (3, 200_003), (3, 197_120), (2, 70_001), (1, 300), (3, 1_000_003)])
def test_product_forward_equals_debug_forward_with_sh(D, P, gpu_device):
    """The non-debug forward at SH degree >= 1 runs its own compile-time variants of k_preprocess (degree 1 and 3: the
    SH rows of the next block prefetched per wave and moved into LDS without workgroup barriers; 200 003 Gaussians =
    782 blocks on 391 workgroups of two blocks each, the last block partial; 197 120 = 770 full blocks; 1 000 003: six
    blocks per workgroup, digits counted in the kernel);
    the debug forward, which every oracle comparison of this file goes through, takes the general variant with the
    block-wide copy.  Same arithmetic: images, radii and the instance count must be bit-identical."""
    sc = S.make_scene(P, 320, 200, 31 + D, sh_degree=D)
    t, dbg = hip_forward(sc, gpu_device, debug=True)
    t2, prod = hip_forward(sc, gpu_device, debug=False)
    assert int(dbg[0]) == int(prod[0]) > 0
    for i in (1, 2, 3, 4):
        assert torch.equal(dbg[i], prod[i]), i
    t3, again = hip_forward(sc, gpu_device, debug=False)          # (speculative this time)
    for i in (1, 2, 3, 4):
        assert torch.equal(dbg[i], again[i]), i


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [1, 3])
def test_product_sh_variants_against_the_oracle(D, mode, gpu_device):
    """The compile-time k_preprocess variants of the product's inputs at SH degree 1 and 3 (rows of the next block
    prefetched per wave, no workgroup barriers) DIRECTLY against the oracle, not through the library's own debug
    forward: a non-debug forward of 200 003 Gaussians (782 blocks, the last one partial), every stage of check_forward
    -- radii, means2D, depths, conics, colours from SH, clamp flags, keys, lists, ranges, n_contrib, images -- and all
    nine gradient groups (the backward reads the SH rows and the clamp flags the variant wrote)."""
    P, W, H = 200_003, 320, 200
    sc = S.make_scene(P, W, H, 31 + D, sh_degree=D)
    O.set_threads(min(O.max_threads(), 16))
    fr = oracle_forward(sc, mode)
    G.set_binning_capacity_hint(0)
    for k in range(2):                                             # synchronous, then speculative
        t, fwd = hip_forward(sc, gpu_device, debug=False, ref_rects=(mode == "reference"))
        check_forward(sc, fr, fwd, gpu_device, debug=False)
    dcol, dacc = masked_grads(W, H, 31 + D, fr.fragile)
    ref = O.backward(fr, sc, dcol, dacc)
    got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device, debug=False)
    for k in GRAD_NAMES:
        grad_close(got[k], ref[k], k, outlier_frac=2e-6)


@pytest.mark.parametrize("knob", ["GSR_SORT_BALLOT_RANK", "GSR_DEPTH_HIST_PASS", "GSR_TILE_SORT_LSD",
                                  "GSR_TILE_SORT_LSD,GSR_SORT_BALLOT_RANK", "GSR_TILE_SORT_LSD,GSR_RANGES_FROM_KEYS",
                                  "GSR_SORT_TWO_LEVEL_SCAN", "GSR_TILE_SORT_LSD,GSR_SORT_TWO_LEVEL_SCAN"])
def test_sort_fallback_paths(knob, gpu_device):
    """The radix scatter ranks with returning LDS atomics only after a one-time probe of the hardware's conflict
    order; GSR_SORT_BALLOT_RANK=1 forces the ballot-match variant the library falls back to.  GSR_DEPTH_HIST_PASS=1
    makes the depth sort count its digits itself instead of taking the histograms k_preprocess counted;
    GSR_TILE_SORT_LSD=1 sorts the instances in two LSD passes (histogram, scan, scatter each + a range kernel: what
    sorts beyond 16 M pairs and 32-bit keys take) instead of the bucket form (top eight bits, then one launch that
    finishes every bucket and writes the ranges); with it, GSR_RANGES_FROM_KEYS=1 derives the tile ranges from the
    sorted keys instead of the last pass's counts;
    GSR_SORT_TWO_LEVEL_SCAN=1 scans the tile sort's digit counts in two launches as sorts beyond 8 M pairs do.  All are
    read once per process, so the check runs in a child process: bit-exact lists against the oracle there too
    (three forwards: the library-owned histogram buffers alternate between calls)."""
    import subprocess
    import sys
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, gs_livm_amd as G\n"
        "from gs_livm_amd import synthetic as S\n"
        "from oracle import oracle as O\n"
        "from helpers import hip_forward\n"
        "sc = S.make_scene(40000, 500, 300, 6, sh_degree=1)\n"
        "fr = O.forward(sc, tight=True)\n"
        "u = lambda x: x.cpu().numpy().view(np.uint32)\n"
        "for rep in range(3):\n"
        "    t, fwd = hip_forward(sc, torch.device('cuda:0'))\n"
        "    v = G.state_views(fwd[5], fwd[6], fwd[7], 40000, fwd[0], 500, 300)\n"
        "    assert fwd[0] == fr.R and np.array_equal(u(v['point_list']), fr.point_list)\n"
        "    assert np.array_equal(u(v['ranges']), fr.ranges)\n"
        "print('fallback ok')\n") % (os.path.dirname(GOLDEN.rstrip('/').rsplit('/', 1)[0]), os.path.dirname(GOLDEN))
    env = dict(os.environ, **{k: "1" for k in knob.split(",")})
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fallback ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("knob", ["GSR_BLEND_BACKWARD_TILES", "GSR_BLEND_BACKWARD_QUADS", "GSR_BWD_IMAGE_ORDER",
                                  "GSR_SYNC_FORWARD", "GSR_GBWD_ALL"])
def test_blend_backward_kernel_variants(knob, gpu_device):
    """The blend backward has two kernels -- one wave per tile (four pixels per lane) for frames of >= 3072 tiles, one
    wave per 8x8 quad below -- and takes the tiles longest walk first.  The size rule alone would leave the tile
    kernel untested on the small scenes the oracle can check in full and the quad kernel untested on large frames, so
    each variant is forced on both (the knobs are read once per process: child process), gradients against the oracle;
    GSR_SYNC_FORWARD=1 = every forward synchronous; GSR_GBWD_ALL=1 = the per-Gaussian backward walks its chain for
    every visible Gaussian, not only for those the blend backward left records for."""
    import subprocess
    import sys
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, gs_livm_amd as G\n"
        "from gs_livm_amd import synthetic as S\n"
        "from oracle import oracle as O\n"
        "from helpers import hip_forward, hip_backward, grad_close, conic_condition\n"
        "dev = torch.device('cuda:0')\n"
        "for (P, W, H, seed, D) in ((300, 70, 50, 11, 3), (6000, 320, 200, 16, 0), (40000, 500, 300, 6, 1), (7, 33, 17, 3, 1),\n"
        "                           (60000, 1300, 800, 8, 0)):\n"
        "    sc = S.make_scene(P, W, H, seed, sh_degree=D)\n"
        "    if P == 6000:\n"
        "        sc['means3D'][:20, 2] = 1.0; sc['means3D'][:20, :2] *= 0.2; sc['scales'][:20] = 0.29\n"
        "    O.set_threads(min(O.max_threads(), 16))\n"
        "    fr = O.forward(sc)\n"
        "    keep = (fr.fragile == 0).astype(np.float32)[None]\n"
        "    dcol, dacc = S.make_upstream_grads(W, H, seed)\n"
        "    dcol, dacc = dcol * keep, dacc * keep\n"
        "    ref = O.backward(fr, sc, dcol, dacc)\n"
        "    cond = conic_condition(fr.conic_opacity)  # the conditioning-aware bound of helpers.grad_close\n"
        "    for rep in range(2):\n"
        "        t, fwd = hip_forward(sc, dev, debug=False)\n"
        "        got = hip_backward(sc, t, fwd, dcol, dacc, dev, debug=False)\n"
        "        for k in ref:\n"
        "            grad_close(got[k], ref[k], k, cond=cond)\n"
        "print('variant ok')\n") % (os.path.dirname(GOLDEN.rstrip('/').rsplit('/', 1)[0]), os.path.dirname(GOLDEN))
    env = dict(os.environ, **{knob: "1"})
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "variant ok" in out.stdout, out.stderr[-2000:]


def test_randomised_scenes(gpu_device):
    """Twelve seeded random configurations -- image size, field of view, camera yaw / position, SH degree, Gaussian
    count, anisotropy and opacity ranges, background, scale modifier, non-unit quaternions -- through the full
    forward + backward comparison: integer stages bit-exact, images to 1e-4, gradients to the conditioning-aware
    bound of helpers.grad_close (the scenes contain nearly singular conics and screen-filling splats)."""
    _random_scenes(np.random.default_rng(20240611), 12, gpu_device)


def _random_scene(rng, case, pmax=30_000):
    W, H = int(rng.integers(17, 700)), int(rng.integers(9, 420))
    P = int(rng.integers(50, pmax))
    D = int(rng.integers(0, 4))
    seed = 1000 + case
    g = S.make_gaussians(P, seed, sh_degree=D, fovx_deg=float(rng.uniform(35, 100)), aspect=W / H,
                         zmin=float(rng.uniform(0.3, 2.0)), zmax=float(rng.uniform(3.0, 60.0)))
    cam = S.make_camera(W, H, fovx_deg=float(rng.uniform(35, 100)), yaw_deg=float(rng.uniform(-25, 25)),
                        position=tuple(rng.uniform(-0.5, 0.5, 3)))
    sc = dict(g, **cam, bg=rng.uniform(0, 1, 3).astype(np.float32), colors_precomp=None, cov3D_precomp=None,
              scale_modifier=float(rng.uniform(0.5, 1.5)))
    sc["scales"] = (sc["scales"] * rng.uniform(0.5, 2.0, (P, 3))).astype(np.float32)      # stronger anisotropy
    sc["rotations"] = (sc["rotations"] * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32)  # used as given (A.3)
    sc["opacities"] = rng.uniform(0.0, 1.0, (P, 1)).astype(np.float32) ** float(rng.uniform(0.5, 3.0))
    return sc, seed


def _random_scenes(rng, ncases, gpu_device):
    """(also driven with other generator seeds by tools/soak_random_scenes.py)"""
    for case in range(ncases):
        sc, seed = _random_scene(rng, case)
        for mode in MODES:
            _full_check(sc, gpu_device, seed=seed, stress=True, mode=mode)


def _random_near_far(rng, ncases, gpu_device):
    """Random scenes (as above, plus a stack of large opaque splats in front of every other one so that some tiles
    saturate early) binned near/far with a random budget, with and without far-chain speculation: bit-identical to
    the one-chain frame of the same library (_check_near_far_against_one_chain).  Also driven by
    tools/soak_random_scenes.py, under the knobs of test_far_speculation_variants."""
    try:
        for case in range(ncases):
            sc, seed = _random_scene(rng, case, pmax=60_000)
            if case % 2:
                k = min(int(rng.integers(8, 80)), sc["means3D"].shape[0])
                sc["means3D"][:k, :2] *= 0.2
                sc["means3D"][:k, 2] = rng.uniform(0.6, 1.2, k).astype(np.float32)
                sc["scales"][:k] = np.float32(0.29 / max(sc["scale_modifier"], 1.0))
                sc["opacities"][:k] = 0.97
            for spec in (None, True):
                _check_near_far_against_one_chain(sc, gpu_device, int(rng.integers(1, 120)), speculate_far=spec)
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


def test_near_far_randomised(gpu_device):
    _random_near_far(np.random.default_rng(20241004), 8, gpu_device)


@pytest.mark.parametrize("mode", MODES)
def test_tiny_images(mode, gpu_device):
    for (W, H) in ((1, 1), (5, 3), (16, 16), (17, 1)):
        sc = S.make_scene(400, W, H, 19, sh_degree=1)
        sc["means3D"][:, :2] *= 0.05  # everything lands on the few pixels there are
        _full_check(sc, gpu_device, seed=19, mode=mode)


def test_mark_visible(gpu_device):
    sc = S.make_scene(3000, 64, 48, 17)
    t = to_dev(sc, gpu_device)
    got = G.mark_visible(t["means3D"], t["viewmatrix"], t["projmatrix"]).cpu().numpy()
    assert np.array_equal(got, O.mark_visible(sc["means3D"], sc["viewmatrix"]))
    assert G.mark_visible(t["means3D"][:0], t["viewmatrix"], t["projmatrix"]).numel() == 0


def test_unsupported_sh_raises(gpu_device):
    sc = S.make_scene(10, 32, 32, 1, sh_degree=1)
    sc["sh_degree"] = 3  # needs 16 coefficients, only 4 provided
    with pytest.raises(G.GsrError, match="SH degree"):
        hip_forward(sc, gpu_device)


def test_autograd_surface_several_views_one_backward(gpu_device):
    """The caller renders several views, sums the losses and runs ONE backward
    (lioOptimization.cpp:1691-1832): N forward blob triples stay alive, gradients of shared leaves add."""
    dev = gpu_device
    g = S.make_gaussians(3000, 21, sh_degree=1, aspect=160 / 96)
    leaves = {k: torch.from_numpy(g[k]).to(dev).requires_grad_(True)
              for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    total = 0.0
    want = {k: 0.0 for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dsh")}
    O.set_threads(1)
    for yaw in (-6.0, 0.0, 7.0):
        cam = S.make_camera(160, 96, yaw_deg=yaw)
        sc = dict(g, **cam, bg=np.ones(3, np.float32), scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None)
        fr = O.forward(sc)
        keep = (fr.fragile == 0).astype(np.float32)
        wc = np.linspace(0.5, 1.5, 3 * 96 * 160, dtype=np.float32).reshape(3, 96, 160) * keep[None]
        wa = np.full((1, 96, 160), 0.3, np.float32) * keep[None]
        ref = O.backward(fr, sc, wc, wa)  # reference: per-view oracle gradients with the same upstream seeds
        for k in want:
            want[k] = want[k] + ref[k].astype(np.float64)
        st = G.GaussianRasterizationSettings(96, 160, cam["tanfovx"], cam["tanfovy"], torch.ones(3, device=dev), 1.0,
                                             torch.from_numpy(cam["viewmatrix"]).to(dev),
                                             torch.from_numpy(cam["projmatrix"]).to(dev), 1,
                                             torch.from_numpy(cam["campos"]).to(dev), False)
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        color, radii, depth, acc = G.GaussianRasterizer(st)(leaves["means3D"], means2D, leaves["opacities"],
                                                            shs=leaves["shs"], scales=leaves["scales"],
                                                            rotations=leaves["rotations"])
        assert color.shape == (3, 96, 160) and depth.shape == (1, 96, 160) and acc.shape == (1, 96, 160)
        assert radii.dtype == torch.int32 and not radii.requires_grad
        assert np.array_equal(radii.cpu().numpy(), fr.radii)
        # the depth term must contribute NO gradient (rasterizer.cu:79, 117-118)
        total = total + (color * torch.from_numpy(wc).to(dev)).sum() + (acc * torch.from_numpy(wa).to(dev)).sum() \
            + 5.0 * depth.sum()
    total.backward()
    for leaf, k in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh")):
        grad_close(leaves[leaf].grad.cpu().numpy(), want[k].astype(np.float32), k)


def test_render_mirror_equals_the_operator_call(gpu_device):
    """G.render (include/gs/gs/render_utils.cuh:13-56) = settings from the Camera + activated model + one rasterizer
    call: same images as calling the operator by hand, and its backward reaches the raw leaves."""
    import math
    dev = gpu_device
    P, W, H, D = 4000, 200, 120, 2
    g = S.make_gaussians(P, 31, sh_degree=D, aspect=W / H)
    raw = dict(xyz=g["means3D"], f_dc=g["shs"][:, :1], f_rest=g["shs"][:, 1:], scaling=np.log(g["scales"]),
               rotation=g["rotations"] * 1.7, opacity=np.log(g["opacities"] / (1 - g["opacities"])))
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in raw.items()}
    model = G.GaussianParameters(t["xyz"], t["f_dc"], t["f_rest"], t["scaling"], t["rotation"], t["opacity"])
    assert model.Get_max_sh_degree() == D
    a = math.radians(5.0)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
    fovx = math.radians(60.0)
    cam = G.Camera(R, (0.0, 0.1, -0.2), fovx, 2.0 * math.atan(math.tan(fovx / 2.0) * H / W), W, H, device=dev)
    bg = torch.tensor([0.2, 0.5, 0.9])
    color, depth, acc = G.render(cam, model, bg, 1.1)
    assert color.shape == (3, H, W) and depth.shape == (1, H, W) and acc.shape == (1, H, W)
    st = G.GaussianRasterizationSettings(H, W, math.tan(fovx * 0.5), math.tan(cam.Get_FoVy() * 0.5), bg.to(dev), 1.1,
                                         cam.Get_world_view_transform(), cam.Get_full_proj_transform(), D,
                                         cam.Get_camera_center(), False)
    with torch.no_grad():
        xyz, op, sc, rot, shs = model.activated()
        c2, _, d2, a2 = G.GaussianRasterizer(st)(xyz, torch.zeros_like(xyz), op, shs=shs, scales=sc, rotations=rot)
    assert torch.equal(color, c2) and torch.equal(depth, d2) and torch.equal(acc, a2)
    (color.sum() + acc.sum()).backward()
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert float(model._xyz.grad.abs().sum()) > 0 and float(model._features_rest.grad.abs().sum()) > 0
    # precomputed colours through override_color
    col, _, _ = G.render(cam, model, bg, 1.1, override_color=torch.full((P, 3), 0.25, device=dev))
    assert float((col - color).abs().max()) > 0


def test_cpp_libtorch_surface_matches_c_abi_path(gpu_device):
    """The C++/LibTorch binding GS-LIVM would link (csrc/torch_binding.cpp): RasterizeGaussiansCUDA /
    ...BackwardCUDA give bit-identical results to the ctypes route (same C ABI underneath), and the
    GaussianRasterizer module + autograd::Function reproduce them through loss.backward()."""
    dev = gpu_device
    T = G.torch_ops()
    sc = S.make_scene(4000, 210, 130, 23, sh_degree=2)
    t, fwd = hip_forward(sc, dev)
    e = torch.empty(0, device=dev)
    out = T.RasterizeGaussiansCUDA(t["bg"], t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e,
                                   t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], 130, 210, t["shs"],
                                   2, t["campos"], False, False)
    assert T.last_num_rendered() == fwd[0] and out[0] >= fwd[0]  # (the binning key of a speculative forward >= the count)
    for a, b in zip(out[1:5], fwd[1:5]):
        assert torch.equal(a, b)
    dcol, dacc = S.make_upstream_grads(210, 130, 23)
    dc, da = torch.from_numpy(dcol).to(dev), torch.from_numpy(dacc).to(dev)
    gb = T.RasterizeGaussiansBackwardCUDA(t["bg"], t["means3D"], out[4], e, t["scales"], t["rotations"], 1.0, e,
                                          t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], dc, da,
                                          t["shs"], 2, t["campos"], out[5], out[0], out[6], out[7], False)
    ref = hip_backward(sc, t, fwd, dcol, dacc, dev)
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations")
    for n, g in zip(names, gb):
        assert np.array_equal(g.cpu().numpy(), ref[n]), n
    # module + autograd
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    st = T.GaussianRasterizationSettings(130, 210, sc["tanfovx"], sc["tanfovy"], t["bg"], 1.0, t["viewmatrix"],
                                         t["projmatrix"], 2, t["campos"], False)
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, depth, acc = T.GaussianRasterizer(st).forward(leaves["means3D"], means2D, leaves["opacities"],
                                                                shs=leaves["shs"], scales=leaves["scales"],
                                                                rotations=leaves["rotations"])
    assert torch.equal(color, fwd[1]) and torch.equal(radii, fwd[4]) and not radii.requires_grad
    ((color * dc).sum() + (acc * da).sum() + depth.sum()).backward()
    for leaf, n in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh")):
        assert np.array_equal(leaves[leaf].grad.cpu().numpy(), ref[n].reshape(leaves[leaf].shape)), n
    assert np.array_equal(means2D.grad.cpu().numpy(), ref["dL_dmeans2D"])
    vis = T.markVisible(t["means3D"], t["viewmatrix"], t["projmatrix"])
    assert np.array_equal(vis.cpu().numpy(), O.mark_visible(sc["means3D"], sc["viewmatrix"]))


# ----------------------------- full-size, size-independent properties -----------------------------
@pytest.fixture(scope="module")
def c3(gpu_device):
    P, W, H, seed = S.CONFIGS["C3"]
    sc = S.make_scene(P, W, H, seed)
    t, fwd = hip_forward(sc, gpu_device, debug=False)
    return sc, t, fwd


def test_c3_structure(c3, gpu_device):
    sc, t, fwd = c3
    P, W, H = 2_000_000, 1920, 1080
    R = fwd[0]
    v = G.state_views(fwd[5], fwd[6], fwd[7], P, R, W, H)
    tiles = v["tiles_touched"].long()
    assert int(tiles.sum()) == R
    # ranges: (0, 0) for empty tiles, otherwise back-to-back in tile order, covering [0, R)
    rg = v["ranges"].long()
    ln = rg[:, 1] - rg[:, 0]
    assert int(ln.min()) >= 0 and int(ln.sum()) == R
    nz = ln > 0
    assert torch.equal(rg[nz, 0], (torch.cumsum(ln, 0) - ln)[nz]) and not bool(rg[~nz].any())
    # inside a tile: ascending depth bits, ties in ascending Gaussian id (= the reference's 64-bit key order);
    # state_views recomposes the keys from the tile of each position (via ranges) and the Gaussian's depth bits
    keys, pl = v["keys"], v["point_list"].long()
    assert bool((keys[1:] >= keys[:-1]).all())                              # sortedness (keys < 2^45: signed ok)
    tie = keys[1:] == keys[:-1]
    assert bool((pl[1:][tie] > pl[:-1][tie]).all())                         # stability
    # every Gaussian appears exactly tiles_touched times, on a full rectangle of tiles_touched distinct tiles
    assert torch.equal(torch.bincount(pl, minlength=P), tiles)
    tid = keys >> 32
    tx, ty = tid % 120, tid // 120
    big = torch.full((P,), 1 << 20, device=pl.device, dtype=torch.long)
    x0 = big.clone().scatter_reduce(0, pl, tx, "amin")
    y0 = big.clone().scatter_reduce(0, pl, ty, "amin")
    x1 = (-big).scatter_reduce(0, pl, tx, "amax")
    y1 = (-big).scatter_reduce(0, pl, ty, "amax")
    has = tiles > 0
    assert torch.equal(((x1 - x0 + 1) * (y1 - y0 + 1))[has], tiles[has])
    uniq = torch.unique(tid * P + pl)                                       # no (tile, Gaussian) pair twice
    assert uniq.numel() == R
    acc, fT = fwd[3][0], v["final_T"]
    assert float((acc + fT - 1).abs().max()) < 1e-4                         # telescoping sum: sum alpha T = 1 - T_final
    assert bool((fwd[1] >= 0).all()) and bool(torch.isfinite(fwd[1]).all()) and bool(torch.isfinite(fwd[2]).all())


def test_c3_per_gaussian_stage_matches_oracle_on_a_subsample(c3, gpu_device):
    """The per-Gaussian stage is independent per Gaussian: every 97th Gaussian run alone through the oracle
    must reproduce the full run's radii / xy / depth / conic / tile count bit for bit."""
    sc, t, fwd = c3
    idx = np.arange(0, 2_000_000, 97)
    sub = dict(sc)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sub[k] = sc[k][idx]
    fr = O.forward(sub, keep_handle=False, tight=True)
    v = G.state_views(fwd[5], fwd[6], fwd[7], 2_000_000, fwd[0], 1920, 1080)
    ti = torch.from_numpy(idx).to(gpu_device)
    assert np.array_equal(fwd[4][ti].cpu().numpy(), fr.radii)
    assert np.array_equal(_u32(v["tiles_touched"][ti]), fr.tiles_touched)
    vis = fr.radii > 0
    sp = v["splats"][ti].cpu().numpy()
    assert np.array_equal(sp[vis, 0:2], fr.means2D[vis]) and np.array_equal(sp[vis, 9], fr.depths[vis])
    assert np.array_equal(sp[vis][:, 2:5], fr.conic_opacity[vis][:, :3])


def test_c3_determinism_and_backward_linearity(c3, gpu_device):
    sc, t, fwd = c3
    dev = gpu_device
    t2, fwd2 = hip_forward(sc, dev, debug=False)
    for a, b in zip(fwd[1:5], fwd2[1:5]):
        assert torch.equal(a, b)                                            # forward is bitwise reproducible
    W, H = 1920, 1080
    g1c, g1a = S.make_upstream_grads(W, H, 101)
    g2c, g2a = S.make_upstream_grads(W, H, 202)
    A = hip_backward(sc, t, fwd, g1c, g1a, dev, debug=False)
    A2 = hip_backward(sc, t2, fwd2, g1c, g1a, dev, debug=False)
    for k in A:
        assert np.array_equal(A[k], A2[k]), k                               # backward too (no atomics)
    B = hip_backward(sc, t, fwd, g2c, g2a, dev, debug=False)
    Cc = hip_backward(sc, t, fwd, 2.0 * g1c - 3.0 * g2c, 2.0 * g1a - 3.0 * g2a, dev, debug=False)
    for k in A:                                                             # backward is linear in the upstream grads
        lin = 2.0 * A[k].astype(np.float64) - 3.0 * B[k].astype(np.float64)
        scale = np.abs(lin).max() + 1e-30
        assert np.abs(Cc[k] - lin).max() <= 2e-4 * scale, k
    A3 = hip_backward(sc, t, fwd, g1c, g1a, dev, debug=False)               # 4th backward over the same blobs:
    for k in A:                                                             # the bookkeeping flags were left clean
        assert np.array_equal(A[k], A3[k]), k
    vis = fwd[4].cpu().numpy() > 0
    assert not A["dL_dmeans3D"][~vis].any() and np.isfinite(A["dL_dmeans3D"]).all()


@pytest.mark.parametrize("mode", MODES)
def test_c2_full_parity_with_oracle(mode, gpu_device):
    """BASELINE C2 (500 k Gaussians, 1280x720): complete forward parity incl. tile ranges, all threads of the host."""
    P, W, H, seed = S.CONFIGS["C2"]
    sc = S.make_scene(P, W, H, seed)
    O.set_threads(min(O.max_threads(), 16))  # the GPU box's CPU share
    fr = oracle_forward(sc, mode, keep_handle=False)
    t, fwd = hip_forward(sc, gpu_device, debug=False, ref_rects=(mode == "reference"))
    check_forward(sc, fr, fwd, gpu_device, debug=False)


def test_c3_full_parity_with_oracle(c3, gpu_device):
    """BASELINE C3 at full size (2 M Gaussians, 1920x1080) against the oracle itself, not only through properties:
    every forward stage in the reference's binning (tiles_touched, num_rendered, keys, point_list, ranges,
    n_contrib bit-exact against the reference-definition frame), the culled default against the oracle's tight
    frame, and all nine gradient arrays of the backward."""
    sc, t_c, fwd_c = c3
    P, W, H, seed = S.CONFIGS["C3"]
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc)                                   # the reference's definition
    t, fwd = hip_forward(sc, gpu_device, ref_rects=True)
    check_forward(sc, fr, fwd, gpu_device)
    dcol, dacc = masked_grads(W, H, seed, fr.fragile)
    ref = O.backward(fr, sc, dcol, dacc)
    got = hip_backward(sc, t, fwd, dcol, dacc, gpu_device, debug=False)
    for k in GRAD_NAMES:   # (16-thread oracle: atomic-order noise of its own, see grad_close)
        grad_close(got[k], ref[k], k, outlier_frac=1e-6)
    R_ref = fr.R
    fr.close()
    del fr, fwd
    ft = O.forward(sc, keep_handle=False, tight=True)    # the product's default binning
    assert ft.R < R_ref
    check_forward(sc, ft, fwd_c, gpu_device, debug=False)
    got_c = hip_backward(sc, t_c, fwd_c, dcol, dacc, gpu_device, debug=False)
    for k in GRAD_NAMES:                                 # same gradients from the shorter lists
        grad_close(got_c[k], ref[k], k, outlier_frac=1e-6)


def test_c4_eight_views_forward_parity(gpu_device):
    """BASELINE C4's workload on one GPU: the eight keyframe views (yaw offsets C4_YAWS_DEG) of the 2 M-Gaussian scene
    at 1920x1080, each compared stage by stage with the oracle -- all eight in the reference's binning, the first
    and the last also in the product's culled default.  (The 8-GPU run shards exactly these views, one per rank.)"""
    P, W, H, seed = S.CONFIGS["C4"]
    g = S.make_gaussians(P, seed, aspect=W / H)
    O.set_threads(min(O.max_threads(), 16))
    for i, yaw in enumerate(S.C4_YAWS_DEG):
        sc = dict(g, **S.make_camera(W, H, yaw_deg=yaw), bg=np.ones(3, np.float32), scale_modifier=1.0,
                  colors_precomp=None, cov3D_precomp=None)
        for mode in (MODES if i in (0, len(S.C4_YAWS_DEG) - 1) else MODES[:1]):
            fr = oracle_forward(sc, mode, keep_handle=False)
            t, fwd = hip_forward(sc, gpu_device, debug=False, ref_rects=(mode == "reference"))
            check_forward(sc, fr, fwd, gpu_device, debug=False)
            assert fr.R > 10_000_000
            del fr, t, fwd


def test_backward_without_the_covariance_gradient(gpu_device):
    """dL_dcov3D may be NULL when the covariance comes from scales and rotations (include/gsraster.h, gsr_backward): it
    is then an intermediate nobody reads, and the operator's autograd node does not have it written.  Every other
    gradient is bit-identical to the call that asks for it."""
    sc = S.make_scene(20_000, 320, 200, 8, sh_degree=1)
    t, fwd = hip_forward(sc, gpu_device, debug=False)
    R, color, depth, acc, radii, geom, binning, img = fwd
    dcol, dacc = S.make_upstream_grads(320, 200, 8)
    args = (t["bg"], t["means3D"], radii, t["colors_precomp"], t["scales"], t["rotations"], 1.0, t["cov3D_precomp"],
            t["viewmatrix"], t["projmatrix"], sc["tanfovx"], sc["tanfovy"], torch.from_numpy(dcol).to(gpu_device),
            torch.from_numpy(dacc).to(gpu_device), t["shs"], 1, t["campos"], geom, R, binning, img, False)
    full = G.rasterize_backward(*args)
    lean = G.rasterize_backward(*args, want_cov3D=False)
    assert lean[4] is None and full[4].abs().max() > 0
    for k, (a, b) in enumerate(zip(full, lean)):
        if k != 4:
            assert torch.equal(a, b), k


def test_views_rendered_from_several_threads_one_backward(gpu_device):
    """gs_livm_amd.multiview.ViewThreads: the K views of an iteration rendered from T host threads on T streams (the
    reference's rendering threads), every forward a speculative split frame where the scene allows, then ONE
    backward from the calling thread.  Images are bit-identical to the same views rendered one after the other on the
    calling thread; the leaves' gradients agree to the last bits (autograd adds the views' gradients in the order their
    backwards finish, which several streams do not fix) and, within the usual tolerance, with the sum of the seven views'
    oracle gradients (each view's upstream gradients masked by that view's fragile pixels)."""
    from gs_livm_amd import multiview as MV
    dev = gpu_device
    W, H = 320, 208
    g = _stack_scene(W=W, H=H)
    yaws = [-18.0, -9.0, -3.0, 0.0, 3.0, 9.0, 18.0]
    bg = torch.ones(3, device=dev)
    rasters = []
    for yaw in yaws:
        cam = S.make_camera(W, H, yaw_deg=yaw)
        rasters.append(G.GaussianRasterizer(G.GaussianRasterizationSettings(
            H, W, cam["tanfovx"], cam["tanfovy"], bg, 1.0, torch.from_numpy(cam["viewmatrix"]).to(dev),
            torch.from_numpy(cam["projmatrix"]).to(dev), 0, torch.from_numpy(cam["campos"]).to(dev), False)))
    # per view: upstream gradients masked by its fragile pixels, and its oracle gradients
    O.set_threads(min(O.max_threads(), 8))
    seeds, want = [], None
    for j, yaw in enumerate(yaws):
        sc = dict(g, **S.make_camera(W, H, yaw_deg=yaw), bg=np.ones(3, np.float32), scale_modifier=1.0,
                  colors_precomp=None, cov3D_precomp=None)
        fr = O.forward(sc, tight=True)
        dcol, dacc = masked_grads(W, H, 5 + j, fr.fragile)
        seeds += [torch.from_numpy(dcol).to(dev), torch.from_numpy(dacc).to(dev)]
        ref = O.backward(fr, sc, dcol, dacc)
        ref = {k: x.astype(np.float64) for k, x in ref.items()}
        want = ref if want is None else {k: want[k] + ref[k] for k in ref}

    def run(vt):
        leaves = {k: torch.from_numpy(g[k]).to(dev).requires_grad_(True)
                  for k in ("means3D", "scales", "rotations", "opacities", "shs")}
        images = None
        for it in range(3):                                      # histories settle: speculative, split frames
            for v in leaves.values():
                v.grad = None
            sinks = [torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True) for _ in rasters]
            calls = [lambda r=r, m=m: r(leaves["means3D"], m, leaves["opacities"], shs=leaves["shs"],
                                        scales=leaves["scales"], rotations=leaves["rotations"])
                     for r, m in zip(rasters, sinks)]
            outs = vt.render(calls) if vt is not None else [c() for c in calls]
            torch.autograd.backward([t for o in outs for t in (o[0], o[3])], seeds)
            images = [o[0].detach().clone() for o in outs]
        torch.cuda.synchronize()
        return images, {k: v.grad.clone() for k, v in leaves.items()}

    img1, g1 = run(None)
    vt = MV.ViewThreads(3, dev)
    async_before = G.speculation_stats()["async_far_frames"]
    try:
        img3, g3 = run(vt)
    finally:
        vt.close()
    # while several host threads render, no frame takes the asynchronous far chain (second stream, stream-side waits):
    # the host-decided variant costs nothing beside the other threads' work (include/gsraster.h)
    assert G.speculation_stats()["async_far_frames"] == async_before
    for a, b in zip(img1, img3):
        assert torch.equal(a, b)
    for k in g1:
        scale = float(g1[k].abs().max())
        assert float((g1[k] - g3[k]).abs().max()) <= 2e-6 * scale + 1e-12, k
    # ... and the sum of the seven views' oracle gradients
    for leaf, k in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh")):
        grad_close(g3[leaf].cpu().numpy(), want[k].astype(np.float32), k)
