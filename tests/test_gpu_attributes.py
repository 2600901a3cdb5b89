"""GPU tests of the attribute blend (csrc/render.hip k_attribute_tile through gsr_blend_attributes and
gs_livm_amd.blend_attributes).

1. Against the forward itself, bit for bit: the walk recomputes the forward's alpha and T and accumulates with the
   forward's own fused multiply-add, so attributes = 1 is the silhouette, the splats' view depth the depth image and the
   colours (zero background) the colour image -- the same bits, no tolerance.
2. Against tests/attr_ref.py (float64 on the CPU oracle's frames) for signed attributes, off the oracle's fragile pixels:
   |out - out64| <= B sum w |attr|, B = 8 x the float32 yardstick's worst ratio (attr_ref.B = 2.08e-5)."""
import functools

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi
from gs_livm_amd import synthetic as S

import attr_ref as AR
import contrib_ref as CR
from arena import Arena, offsets
from helpers import hip_forward
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _blend(fwd, attr, W, H, out=None):
    P = int(attr.shape[0])
    return _capi.blend_attributes(P, fwd[0], W, H, attr, fwd[5], fwd[6], fwd[7], out=out)


def _check_against_the_forward(sc, dev, **fwd_kw):
    """acc, depth, colour and (colour, acc) of one scene; returns the number of pixels something was blended into"""
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    _, fwd = hip_forward(sc, dev, debug=False, **fwd_kw)
    v = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], W, H)
    assert _same(_blend(fwd, torch.ones((P, 1), device=dev), W, H), fwd[3])
    z = v["splats"][:, 9].clone()
    z[fwd[4] <= 0] = float("nan")                       # rows the forward culled are never read
    assert _same(_blend(fwd, z[:, None].contiguous(), W, H), fwd[2])
    sc = dict(sc)
    sc["colors_precomp"] = np.random.default_rng(3).uniform(0, 1, (P, 3)).astype(np.float32)
    sc["shs"], sc["bg"] = None, np.zeros(3, np.float32)
    t, fwd = hip_forward(sc, dev, debug=False, **fwd_kw)
    assert _same(_blend(fwd, t["colors_precomp"], W, H), fwd[1])
    rgb1 = torch.cat([t["colors_precomp"], torch.ones((P, 1), device=dev)], 1).contiguous()
    out4 = _blend(fwd, rgb1, W, H)
    assert _same(out4[:3], fwd[1]) and _same(out4[3:], fwd[3])
    return int((fwd[3] > 0).sum())


# ---- 1. against the forward, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CR.SCENES)
def test_scenes_equal_the_forward(cfg, gpu_device):
    assert _check_against_the_forward(CR.scene(*cfg), gpu_device) > 0     # (not vacuous: something was blended)


def test_reference_rectangles_equal_the_forward(gpu_device):
    assert _check_against_the_forward(CR.scene(*CR.SCENES[2]), gpu_device, ref_rects=True) > 0


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 257])
def test_a_transparent_stack_across_sub_chunk_seams(N, gpu_device):
    assert _check_against_the_forward(CR.stack_scene(N, 0.02), gpu_device) == 256


@pytest.mark.parametrize("sigma_px", [100.0, 6.0])
def test_an_opaque_stack_stops_where_the_forward_stopped(sigma_px, gpu_device):
    # the walk is bounded by the tile's longest prefix: only `position < n_contrib` keeps a stopped pixel from taking more
    assert _check_against_the_forward(CR.stack_scene(8, 0.95, sigma_px=sigma_px), gpu_device) == 256


def test_a_splat_on_the_partial_corner_tile(gpu_device):
    assert _check_against_the_forward(CR.splat_scene(70, 50, [[66.3, 48.2]], [2.0], 1.7, 0.8), gpu_device) > 0


def test_near_far_frames_equal_the_forward(gpu_device):
    dev = gpu_device
    sc = S.make_scene(60_000, 640, 400, 16, sh_degree=0)   # the scene of tests/test_gpu_contrib.py's near/far test
    sc["means3D"][:40, 2] = 1.0
    sc["means3D"][:40, :2] *= 0.3
    sc["scales"][:40] = 0.29
    sc["opacities"][:40] = 0.95
    try:
        for near_entries in (4, 64):
            G.set_binning_capacity_hint(0)
            G.set_near_far_hints(near_entries, None)
            assert _check_against_the_forward(sc, dev, near_far=True) > 0
            torch.cuda.synchronize()
            split, n_near, n_far = G.last_near_far()
            assert split and n_near > 0 and n_far > 0
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)


# ---- 2. against float64 ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(cfg):
    sc = CR.scene(*cfg)
    return sc, O.forward(sc)


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_signed_attributes_equal_float64_at_the_bar(cfg, gpu_device):
    sc, fr = _reference(cfg)
    P, W, H = fr.P, fr.W, fr.H
    ok = fr.fragile == 0
    assert (~ok).mean() <= AR.MAX_FRAGILE_SHARE
    _, fwd = hip_forward(sc, gpu_device, debug=False)
    for C in (1, 2, 3, 4):
        at = AR.attributes(P, C)
        out64, scale = AR.blend64(fr, at)
        got = _blend(fwd, torch.from_numpy(at).to(gpu_device), W, H).cpu().numpy()
        assert got.shape == (C, H, W)
        r = AR.worst_ratio(got, out64, scale, ok)
        print("channels %d: worst |d| / sum w |attr| %.3e (bar %.3e)" % (C, r, AR.B))
        assert r <= AR.B
        assert not got[:, ok & (scale[0] == 0)].any()   # nothing blended: exactly zero


# ---- 3. every element is written ---------------------------------------------------------------------------------------------
def test_every_element_is_written_and_uncovered_pixels_read_plus_zero(gpu_device):
    dev = gpu_device
    for cfg in (CR.SCENES[1], CR.SCENES[0]):
        sc = CR.scene(*cfg)
        P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
        _, fwd = hip_forward(sc, dev, debug=False)
        n_contrib = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], W, H)["n_contrib"].view(H, W)
        for C in (1, 3, 4):
            out = torch.full((C * H * W * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(C, H, W)
            got = _blend(fwd, torch.from_numpy(AR.attributes(P, C)).to(dev), W, H, out=out)
            assert got.data_ptr() == out.data_ptr()
            bits = _bits(got)
            assert not (bits == -1).any()               # no element keeps the prefill
            empty = n_contrib == 0
            assert empty.any() and not bits[:, empty].any()   # +0.0, not -0.0


# ---- 4. alignment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["a4", "a8", "a12"])
def test_attributes_and_out_off_sixteen_bytes(mode, gpu_device):
    dev = gpu_device
    sc = CR.scene(*CR.SCENES[0])
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    _, fwd = hip_forward(sc, dev, debug=False)
    for C in (1, 2, 3, 4):
        at = torch.from_numpy(AR.attributes(P, C)).to(dev)
        want = _blend(fwd, at, W, H)
        ar = Arena(dev, offsets(mode))
        a_view, o_view = ar.put("attributes", src=at), ar.put("out", shape=(C, H, W))
        got = _blend(fwd, a_view, W, H, out=o_view)
        assert got.data_ptr() % 16 == int(mode[1:]) and _same(got, want)
        assert ar.guards_intact() is None


# ---- 5. empty inputs ---------------------------------------------------------------------------------------------------------
def test_an_empty_model_and_an_empty_frame_give_zeros(gpu_device):
    dev = gpu_device
    ff = lambda C, H, W: torch.full((C * H * W * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(C, H, W)  # noqa: E731
    sc = CR.splat_scene(33, 17, np.zeros((0, 2)), np.zeros(0), 1.0, 0.5)
    _, fwd = hip_forward(sc, dev, debug=False)
    out = _blend(fwd, torch.empty((0, 3), device=dev), 33, 17, out=ff(3, 17, 33))
    assert out.shape == (3, 17, 33) and not _bits(out).any()
    sc = CR.scene(50, 33, 17, 3, 0)
    sc["means3D"][:, 2] = -np.abs(sc["means3D"][:, 2]) - 1.0   # everything behind the camera: R == 0
    _, fwd = hip_forward(sc, dev, debug=False)
    assert int(fwd[0]) == 0
    out = _blend(fwd, torch.full((50, 2), float("nan"), device=dev), 33, 17, out=ff(2, 17, 33))
    assert not _bits(out).any()


# ---- 6. determinism and the public surface -----------------------------------------------------------------------------------
def test_a_repeated_run_is_bit_equal(gpu_device):
    sc = CR.scene(*CR.SCENES[2])
    P, W, H = sc["means3D"].shape[0], sc["W"], sc["H"]
    _, fwd = hip_forward(sc, gpu_device, debug=False)
    at = torch.from_numpy(AR.attributes(P, 3)).to(gpu_device)
    a, b = _blend(fwd, at, W, H), _blend(fwd, at, W, H)
    assert a.any() and _same(a, b)
    # the public wrapper: the same launch; a [P] vector is one channel
    assert _same(G.blend_attributes(fwd, at, W, H), a)
    assert _same(G.blend_attributes(fwd, at[:, 0].contiguous(), W, H), _blend(fwd, at[:, :1].contiguous(), W, H))
    with pytest.raises(ValueError):
        G.blend_attributes(fwd, torch.zeros((P, 5), device=gpu_device), W, H)
