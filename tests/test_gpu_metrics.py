"""GPU tests of the evaluation pass (csrc/metrics.hip: k_metrics_forward, k_metrics_finalize, k_pack_image_u8,
k_pack_depth_u8) against the restatements in tests/metrics_ref.py.

psnr, ssim, l1 and mse are compared, from identical float32 inputs, with a float64 evaluation at
max(2 e_ref, K 2^-23 magnitude); K is counted from the kernels' arithmetic in the docstring of metrics_ref.py (SSIM and
L1: loss_ref.py's) and is not fitted to what the kernels return.  An infinite psnr is compared for equality.  Every
figure is printed as a JSON line before it is asserted; the worst ratios measured on an MI355X are in DESIGN.md section 2.

Exact assertions (no bar): the running totals are the sequential float64 sum of the per-frame outputs; guards around
every buffer keep their bits at every byte offset and the results do not depend on the address; two runs are bit-equal;
the 8-bit packs equal the CPU restatement byte for byte and write nothing outside a row's own bytes; the LibTorch
route equals the Python route bit for bit; evaluate_keyframes returns what image_metrics returns on render()'s images.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import loss_ref as R
import metrics_ref as M
from arena import PAT, Arena
from gs_livm_amd import synthetic as S

pytestmark = pytest.mark.gpu
GUARD = 0xA5           # byte pattern of the 8-bit buffers
I32 = torch.int32


def _bits(t):
    return t.contiguous().view(I32)


def _run(c, dev, totals=None):
    return G._capi.image_metrics(c["img"].to(dev), c["gt"].to(dev), c["w"].tolist(), totals=totals)


def _hold(c, out4, what, **info):
    res = M.ratios(out4.cpu().tolist(), c["r64"], c["bar"])
    print(json.dumps(dict(what=what, **info, worst_over_bar={k: float("%.4g" % v[3]) for k, v in res.items()},
                          figures={k: ["%.3g" % x for x in v[:3]] for k, v in res.items()},
                          psnr=c["r64"]["psnr"])))
    over = ["%s: err %.3g, e_ref %.3g, bar %.3g: %.3g of the bar" % ((k,) + v) for k, v in res.items() if not v[3] <= 1.0]
    assert not over, "%s over the bar: %s" % (what, "; ".join(over))
    return res


# ---- metrics against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", M.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_metrics_against_float64(name, shape, gpu_device):
    c = M.case(name, shape)
    out4 = _run(c, gpu_device)
    _hold(c, out4, "metrics", gen=name, shape=list(shape))
    assert torch.equal(_bits(out4), _bits(_run(c, gpu_device)))          # run to run
    if name in ("identical", "one_identical_channel"):
        assert float(out4[0]) == math.inf
    if name == "identical":
        assert float(out4[2]) == 0.0 and float(out4[3]) == 0.0
    if name == "decades" and shape[0] == 3:
        # the mean of the per-channel PSNRs (60 dB), which the pooled formula misses by 35 dB
        assert abs(float(out4[0]) - 60.0) < 0.1 and float(out4[0]) - M.psnr_pooled(c["img"], c["gt"]) > 10.0
    # reported, not required: the same arithmetic in a differently built kernel
    out3, _ = G._capi.photometric_loss(c["img"].to(gpu_device), c["gt"].to(gpu_device), c["w"].tolist(), 0.2, want_grad=False)
    print(json.dumps(dict(what="vs photometric_loss", gen=name, shape=list(shape),
                          ssim_bit_equal=bool(_bits(out4[1:2]).equal(_bits(out3[2:3]))),
                          l1_bit_equal=bool(_bits(out4[2:3]).equal(_bits(out3[1:2]))))))


def test_psnr_and_the_package_surface(gpu_device):
    c = M.case("edges", (3, 33, 55))
    img, gt = c["img"].to(gpu_device), c["gt"].to(gpu_device)
    out4 = G.image_metrics(img, gt)
    assert out4.shape == (4,) and out4.is_cuda and torch.equal(_bits(out4), _bits(_run(c, gpu_device)))
    p = G.psnr(img, gt)
    assert p.dim() == 0 and float(p) == float(out4[0])
    chw = img.permute(1, 2, 0).contiguous().permute(2, 0, 1)             # a non-contiguous view of the same image
    assert not chw.is_contiguous() and torch.equal(_bits(G.image_metrics(chw, gt)), _bits(out4))


# ---- totals -----------------------------------------------------------------------------------------------------------
FRAMES = [("noise", (3, 33, 55)), ("edges", (3, 33, 55)), ("tiny_noise", (3, 33, 55)), ("dark", (3, 33, 55)),
          ("decades", (3, 33, 55))]


@pytest.mark.parametrize("with_infinite", [False, True], ids=["finite", "one_infinite_frame"])
def test_totals_are_the_sequential_float64_sum(with_infinite, gpu_device):
    frames = list(FRAMES)
    if with_infinite:
        frames[2] = ("one_identical_channel", (3, 33, 55))
    totals = torch.zeros(4, dtype=torch.float64, device=gpu_device)
    outs = []
    for name, shape in frames:
        outs.append(_run(M.case(name, shape), gpu_device, totals=totals).cpu())
    want = [0.0, 0.0, 0.0, 0.0]
    for o in outs:                                        # python floats are IEEE doubles: float(o[k]) widens exactly
        want = [want[0] + float(o[0]), want[1] + float(o[1]), want[2] + float(o[2]), want[3] + 1.0]
    got = totals.cpu()
    assert torch.equal(got.view(torch.int64), torch.tensor(want, dtype=torch.float64).view(torch.int64)), (got, want)
    assert float(got[3]) == 5.0
    assert len({float(o[0]) for o in outs}) == 5          # five different frames
    if with_infinite:
        assert float(got[0]) == math.inf and math.isfinite(float(got[1])) and math.isfinite(float(got[2]))
    # without totals the four outputs are the same
    for (name, shape), o in zip(frames, outs):
        assert torch.equal(_bits(_run(M.case(name, shape), gpu_device).cpu()), _bits(o))


# ---- guarded buffers ----------------------------------------------------------------------------------------------------
OFFS = {"a0": dict(img=0, gt=0, out4=0, totals=0, ws=0), "a4": dict(img=4, gt=4, out4=4, totals=0, ws=4),
        "a8": dict(img=8, gt=8, out4=8, totals=8, ws=8), "a12": dict(img=12, gt=12, out4=12, totals=8, ws=12),
        "mix": dict(img=0, gt=4, out4=8, totals=8, ws=12), "xim": dict(img=12, gt=8, out4=4, totals=0, ws=0)}


@pytest.mark.parametrize("mode", list(OFFS))
@pytest.mark.parametrize("name,shape", [("edges", (3, 33, 55)), ("noise", (1, 65, 109))])
def test_misaligned_guarded_buffers_and_an_exact_workspace(name, shape, mode, gpu_device):
    """img, gt, out4, totals and the workspace at byte offsets 0 / 4 / 8 / 12 (totals 0 / 8) inside NaN-patterned
    allocations, the workspace EXACTLY gsr_image_metrics_workspace bytes: every guard keeps its bits, every output word
    is written and the results are bit-equal to the aligned run's."""
    L = G._capi.lib()
    c = M.case(name, shape)
    Cn, H, W = shape
    nbytes = int(L.gsr_image_metrics_workspace(Cn, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    A = Arena(gpu_device, lambda nm, i: OFFS[mode][nm])
    A.put("img", c["img"])
    A.put("gt", c["gt"])
    A.put("out4", shape=(4,))
    tot32 = A.put("totals", shape=(8,))
    A.put("ws", shape=(nbytes // 4,))
    totals = tot32.view(torch.float64)
    totals.copy_(torch.tensor([1.5, -2.0, 0.25, 7.0], dtype=torch.float64))
    win = (C.c_float * 11)(*c["w"].tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = L.gsr_image_metrics(Cn, H, W, A.ptr("img"), A.ptr("gt"), win, A.ptr("out4"), A.ptr("totals"), A.ptr("ws"),
                               nbytes, stream)
    torch.cuda.synchronize()
    assert code == 0, L.gsr_last_error()
    assert A.guards_intact() is None, "guard of %s overwritten" % A.guards_intact()
    assert torch.equal(A.t["img"].cpu(), c["img"]) and torch.equal(A.t["gt"].cpu(), c["gt"])
    out4 = A.t["out4"].clone()
    assert not bool((_bits(out4) == PAT).any()) and not bool((_bits(A.t["ws"]) == PAT).any())
    ref = _run(c, gpu_device)
    assert torch.equal(_bits(out4), _bits(ref))
    o = out4.cpu()
    want = torch.tensor([1.5 + float(o[0]), -2.0 + float(o[1]), 0.25 + float(o[2]), 8.0], dtype=torch.float64)
    assert torch.equal(totals.cpu().view(torch.int64), want.view(torch.int64))
    _hold(c, out4, "guarded", gen=name, shape=list(shape), mode=mode)


def test_refusals_write_nothing(gpu_device):
    L = G._capi.lib()
    Cn, H, W = 3, 33, 55
    nbytes = int(L.gsr_image_metrics_workspace(Cn, H, W))
    A = Arena(gpu_device, lambda nm, i: 0)
    img, gt = R.noise((Cn, H, W))
    A.put("img", img)
    A.put("gt", gt)
    A.put("out4", shape=(4,))
    A.put("totals", shape=(8,))
    A.put("ws", shape=(nbytes // 4,))
    win = (C.c_float * 11)(*R.reference_window_1d().tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda c, h, w, im, nb: L.gsr_image_metrics(c, h, w, im, A.ptr("gt"), win, A.ptr("out4"), A.ptr("totals"),  # noqa: E731
                                                        A.ptr("ws"), nb, stream)
    assert call(Cn, H, W, A.ptr("img"), nbytes - 1) == -1
    assert call(Cn, H, W, None, nbytes) == -1
    assert call(0, H, W, A.ptr("img"), nbytes) == -1
    out8 = torch.full((64,), GUARD, dtype=torch.uint8, device=gpu_device)
    assert L.gsr_pack_image_u8(2, 4, A.ptr("img"), 1, C.c_void_p(out8.data_ptr()), 11, stream) == -1
    assert L.gsr_pack_depth_u8(2, 4, A.ptr("img"), C.c_float(0.0), C.c_void_p(out8.data_ptr()), 4, stream) == -1
    torch.cuda.synchronize()
    for k in ("out4", "totals", "ws"):
        assert bool((A.buf[k] == PAT).all()), "%s written by a refused call" % k
    assert bool((out8 == GUARD).all())
    assert call(Cn, H, W, A.ptr("img"), nbytes) == 0
    torch.cuda.synchronize()
    assert not bool((_bits(A.t["out4"]) == PAT).any())


# ---- 8-bit packs ----------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = (1, 2, 3, 4, 5, 63, 64, 65), (1, 3)


def _fill(pool, count, start):
    idx = (start + np.arange(count)) % len(pool)
    return torch.from_numpy(pool[idx].copy())


def _guarded_u8(dev, H, row_bytes, pitch, base):
    """(buffer, first byte): room for H rows `pitch` apart whose LAST row has only its own row_bytes, 16 guard bytes in
    front (+ base) and behind."""
    n = 16 + base + (H - 1) * pitch + row_bytes + 16
    buf = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, 16 + base


def _expect(buf_len, first, H, row_bytes, pitch, rows):
    want = torch.full((buf_len,), GUARD, dtype=torch.uint8)
    for y in range(H):
        want[first + y * pitch:first + y * pitch + row_bytes] = rows[y].reshape(-1)
    return want


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_pack_image_bytes_pitches_offsets_and_orders(W, H, gpu_device):
    """Bit-exact against the Torch restatement at every pitch in {3W, 3W+1, 3W+2, 3W+3, 6W}, output base offset 0..3,
    both channel orders, and the right half of a side-by-side buffer (base + 3W at pitch 6W); every byte outside the
    3W written bytes of each row keeps its guard pattern."""
    L = G._capi.lib()
    pool = M.unit_pool()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_cases = 0
    pitches = sorted({3 * W, 3 * W + 1, 3 * W + 2, 3 * W + 3, 6 * W})     # (W = 1: 3W + 3 IS 6W)
    for pitch in pitches:
        for base in range(4):
            for bgr in (0, 1):
                for half in ((0, 3 * W) if pitch == 6 * W else (0,)):
                    img = _fill(pool, 3 * H * W, 97 * n_cases + 13 * W + H).view(3, H, W)
                    src = torch.empty(3 * H * W + 3, dtype=torch.float32, device=gpu_device)[(n_cases % 4):][:3 * H * W]
                    src.copy_(img.reshape(-1))                               # (input base at 0 / 4 / 8 / 12 bytes too)
                    buf, first = _guarded_u8(gpu_device, H, 3 * W, pitch, base + half)
                    code = L.gsr_pack_image_u8(H, W, C.c_void_p(src.data_ptr()), bgr, C.c_void_p(buf.data_ptr() + first),
                                               pitch, stream)
                    assert code == 0, L.gsr_last_error()
                    want = _expect(buf.numel(), first, H, 3 * W, pitch, M.to_u8(img, bgr=bool(bgr)))
                    assert torch.equal(buf.cpu(), want), (pitch, base, bgr, half)
                    n_cases += 1
    assert n_cases == 8 * (len(pitches) + 1)


def test_pack_image_covers_every_level_and_its_float_neighbours(gpu_device):
    pool = M.unit_pool()
    H, W = 3, 65
    per = 3 * H * W
    seen = 0
    for start in range(0, len(pool), per):
        img = _fill(pool, per, start).view(3, H, W)
        got = G.to_u8(img.to(gpu_device), bgr=False)
        assert got.dtype == torch.uint8 and got.shape == (H, W, 3) and torch.equal(got.cpu(), M.to_u8(img, bgr=False))
        seen += per
    assert seen >= len(pool)
    # the table, as bytes: 0.5 -> 127 (truncated, not rounded), 254.9999 / 255 -> 254, -0.0 / negatives / -inf -> 0, > 1 / inf -> 255
    x = torch.tensor([0.5, np.float32(254.9999 / 255.0), -0.0, -0.25, -math.inf, 1.5, math.inf, 1.0], dtype=torch.float32)
    got = G.to_u8(x[None, None, :].expand(3, 1, -1).contiguous().to(gpu_device), bgr=True).cpu()
    assert got[0, :, 0].tolist() == [127, 254, 0, 0, 0, 255, 255, 255]


def test_nan_packs_to_zero(gpu_device):
    """Asserted on its own, not against Torch (whose cast of NaN is undefined, as the reference's)."""
    img = torch.full((3, 3, 5), 0.5)
    img[0, 1, 2] = math.nan
    img[2, 0, 4] = -math.nan
    got = G.to_u8(img.to(gpu_device), bgr=False).cpu()
    want = torch.full((3, 5, 3), 127, dtype=torch.uint8)
    want[1, 2, 0] = 0
    want[0, 4, 2] = 0
    assert torch.equal(got, want)
    d = torch.full((3, 5), 10.0)
    d[2, 3] = math.nan
    got = G.depth_to_u8(d.to(gpu_device), 50.0).cpu()
    want = torch.full((3, 5), 51, dtype=torch.uint8)
    want[2, 3] = 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_pack_depth_bytes_pitches_and_offsets(W, H, gpu_device):
    L = G._capi.lib()
    pool = M.depth_pool()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_cases = 0
    pitches = sorted({W, W + 1, W + 2, W + 3, 2 * W})                     # (W = 1, 2, 3: 2W is among the others)
    for pitch in pitches:
        for base in range(4):
            for max_depth in (255.0, 50.0):
                d = _fill(pool, H * W, 89 * n_cases + 7 * W + H).view(H, W)
                src = torch.empty(H * W + 3, dtype=torch.float32, device=gpu_device)[(n_cases % 4):][:H * W]
                src.copy_(d.reshape(-1))
                buf, first = _guarded_u8(gpu_device, H, W, pitch, base)
                code = L.gsr_pack_depth_u8(H, W, C.c_void_p(src.data_ptr()), C.c_float(max_depth),
                                           C.c_void_p(buf.data_ptr() + first), pitch, stream)
                assert code == 0, L.gsr_last_error()
                want = _expect(buf.numel(), first, H, W, pitch, M.depth_to_u8(d, max_depth))
                assert torch.equal(buf.cpu(), want), (pitch, base, max_depth)
                n_cases += 1
    assert n_cases == 8 * len(pitches)


def test_pack_depth_covers_every_tie(gpu_device):
    pool = M.depth_pool()
    W = 65
    H = -(-len(pool) // W)
    d = _fill(pool, H * W, 0).view(H, W)
    got = G.depth_to_u8(d.to(gpu_device), 255.0)
    assert got.shape == (H, W) and torch.equal(got.cpu(), M.depth_to_u8(d, 255.0))
    t = torch.tensor([[0.5, 1.5, 2.5, 254.5, 255.5, -0.0, -3.0, math.inf, -math.inf]])
    assert G.depth_to_u8(t.to(gpu_device), 255.0).cpu()[0].tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0]
    assert G.depth_to_u8(t[None].to(gpu_device), 255.0).shape == (1, 9)           # [1,H,W] as render() returns it
    g = torch.Generator().manual_seed(3)
    r = torch.rand((37, 61), generator=g) * 60.0
    assert torch.equal(G.depth_to_u8(r.to(gpu_device)).cpu(), M.depth_to_u8(r, 50.0))   # max_depth defaults to 50


def test_side_by_side_and_column_slices(gpu_device):
    for H, W in ((3, 5), (2, 64), (3, 65)):
        img, gt = R.noise((3, H, W), amplitude=1.2)
        both = G.side_by_side(img.to(gpu_device), gt.to(gpu_device))
        assert both.shape == (H, 2 * W, 3) and both.dtype == torch.uint8
        want = torch.cat([M.to_u8(img), M.to_u8(gt)], dim=1)
        assert torch.equal(both.cpu(), want)
        # each half on its own into a guarded wide buffer: the other half keeps its guard
        for half in (0, 1):
            wide = torch.full((H, 2 * W, 3), GUARD, dtype=torch.uint8, device=gpu_device)
            out = G.to_u8(img.to(gpu_device), bgr=False, out=wide[:, half * W:(half + 1) * W])
            assert out.data_ptr() == wide.data_ptr() + 3 * W * half
            w = torch.full((H, 2 * W, 3), GUARD, dtype=torch.uint8)
            w[:, half * W:(half + 1) * W] = M.to_u8(img, bgr=False)
            assert torch.equal(wide.cpu(), w)
        dw = torch.full((H, 2 * W), GUARD, dtype=torch.uint8, device=gpu_device)
        G.depth_to_u8(img[0].to(gpu_device) * 40.0, out=dw[:, W:])
        w = torch.full((H, 2 * W), GUARD, dtype=torch.uint8)
        w[:, W:] = M.depth_to_u8(img[0] * 40.0, 50.0)
        assert torch.equal(dw.cpu(), w)
    with pytest.raises(ValueError):
        G.to_u8(torch.zeros((3, 4, 4), device=gpu_device), out=torch.zeros((4, 4, 3), dtype=torch.uint8, device=gpu_device).permute(1, 0, 2))
    with pytest.raises(G.GsrError, match="max_depth"):
        G.depth_to_u8(torch.zeros((4, 4), device=gpu_device), max_depth=0.0)


# ---- hosts ------------------------------------------------------------------------------------------------------------------
def test_libtorch_route_equals_the_python_route(gpu_device):
    nx = G.torch_ops().next
    dev = gpu_device
    for name, shape in (("edges", (3, 33, 55)), ("bright", (1, 65, 109)), ("one_identical_channel", (3, 33, 55))):
        c = M.case(name, shape)
        img, gt = c["img"].to(dev), c["gt"].to(dev)
        ta, tb = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
        a, b = nx.image_metrics(img, gt, totals=ta), G.image_metrics(img, gt, totals=tb)
        assert a.shape == (4,) and torch.equal(_bits(a), _bits(b)) and torch.equal(ta.view(torch.int64), tb.view(torch.int64))
        assert torch.equal(_bits(nx.image_metrics(img, gt, window1d=R.symmetric_window_1d())),
                           _bits(G.image_metrics(img, gt, window11=R.symmetric_window_1d())))
        p = nx.psnr(img, gt)
        assert p.dim() == 0 and torch.equal(_bits(p.reshape(1)), _bits(G.psnr(img, gt).reshape(1)))
    img, gt = (t.to(dev) for t in R.noise((3, 33, 65), amplitude=1.3))
    for bgr in (True, False):
        assert torch.equal(nx.to_u8(img, bgr=bgr), G.to_u8(img, bgr=bgr))
    wa = torch.full((33, 130, 3), GUARD, dtype=torch.uint8, device=dev)
    wb = wa.clone()
    nx.to_u8(gt, out=wa[:, 65:])
    G.to_u8(gt, out=wb[:, 65:])
    assert torch.equal(wa, wb) and bool((wa[:, :65] == GUARD).all()) and torch.equal(wa[:, 65:].cpu(), M.to_u8(gt.cpu()))
    d = img[:1] * 45.0
    assert torch.equal(nx.depth_to_u8(d), G.depth_to_u8(d)) and torch.equal(nx.depth_to_u8(d, 20.0), G.depth_to_u8(d, 20.0))
    da = torch.full((33, 70), GUARD, dtype=torch.uint8, device=dev)
    nx.depth_to_u8(d, out=da[:, 3:68])
    assert torch.equal(da[:, 3:68], G.depth_to_u8(d)) and bool((da[:, :3] == GUARD).all()) and bool((da[:, 68:] == GUARD).all())


# ---- evaluate_keyframes -------------------------------------------------------------------------------------------------------
class _Model:
    """The getters render() asks for, over the tensors of a small synthetic map."""

    def __init__(self, g, dev, colour_shift=0.0):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)  # noqa: E731
        self.xyz, self.opacity, self.scales, self.rot = t("means3D"), t("opacities"), t("scales"), t("rotations")
        self.shs = t("shs")
        if colour_shift:
            gen = torch.Generator().manual_seed(17)
            self.shs = self.shs + colour_shift * (torch.rand(self.shs.shape, generator=gen) - 0.5).to(dev)

    def Get_xyz(self): return self.xyz
    def Get_opacity(self): return self.opacity
    def Get_scaling(self): return self.scales
    def Get_rotation(self): return self.rot
    def Get_features(self): return self.shs
    def Get_max_sh_degree(self): return 0


def _keyframes(dev):
    W, H = 70, 50
    g = S.make_gaussians(300, 21, sh_degree=0, aspect=W / H, zmin=2.0, zmax=8.0)
    g["scales"] = (g["scales"] * 4.0).astype(np.float32)
    fovx = math.radians(60.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * H / W)
    cams = []
    for deg in (-2.0, 0.0, 3.0):                                        # three yawed cameras
        a = math.radians(deg)
        Rm = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
        cams.append(G.Camera(Rm, (0.02 * deg, 0.0, 0.0), fovx, fovy, W, H, device=dev))
    return g, cams, torch.full((3,), 0.1, device=dev)


def test_evaluate_keyframes(gpu_device):
    dev = gpu_device
    G.set_binning_capacity_hint(0)
    g, cams, bg = _keyframes(dev)
    model, truth = _Model(g, dev), _Model(g, dev, colour_shift=0.3)
    prev_nf = G.set_near_far_thread(False)   # (one-chain frames: these tiny views must not feed the near-budget rule)
    try:
        with torch.no_grad():
            gts = [G.render(c, truth, bg)[0] for c in cams]
            images = [G.render(c, model, bg)[0] for c in cams]
        seen = []
        res = G.evaluate_keyframes(cams, gts, model, bg, on_frame=lambda i, im, dp: seen.append((i, im.shape, dp.shape)))
        same = G.evaluate_keyframes(cams, images, model, bg)
    finally:
        G.set_near_far_thread(prev_nf)
    assert res["frames"] == 3 and res["rows"].shape == (3, 4) and not res["rows"].is_cuda
    assert seen == [(i, (3, 50, 70), (1, 50, 70)) for i in range(3)]
    w = R.reference_window_1d()
    for i in range(3):
        direct = G.image_metrics(images[i], gts[i]).cpu()
        assert torch.equal(_bits(res["rows"][i]), _bits(direct)), i      # the rows ARE image_metrics on render()'s images
        img, gt = images[i].cpu(), gts[i].cpu()
        r64, r32 = M.metrics(img, gt, w, torch.float64), M.metrics(img, gt, w, torch.float32)
        c = dict(r64=r64, bar=M.bars(r64, r32, M.floors(img, gt, w, r64)))
        _hold(c, res["rows"][i], "evaluate_keyframes", frame=i)
        assert math.isfinite(r64["psnr"]) and 5.0 < r64["psnr"] < 60.0
    tot = res["totals"]
    want = [0.0, 0.0, 0.0]
    for i in range(3):
        want = [want[k] + float(res["rows"][i][k]) for k in range(3)]
    assert [float(tot[k]) for k in range(3)] == want and float(tot[3]) == 3.0
    assert res["mean_psnr"] == float(tot[0]) / 3.0 and res["mean_ssim"] == float(tot[1]) / 3.0
    # ground truths rendered from the SAME model: the forward is bitwise reproducible, asserted through the new path
    assert same["frames"] == 3 and same["mean_psnr"] == math.inf
    for i in range(3):
        row = same["rows"][i]
        assert float(row[0]) == math.inf and float(row[2]) == 0.0 and float(row[3]) == 0.0
        img = images[i].cpu()
        r64, r32 = M.metrics(img, img, w, torch.float64), M.metrics(img, img, w, torch.float32)
        c = dict(r64=r64, bar=M.bars(r64, r32, M.floors(img, img, w, r64)))
        _hold(c, row, "evaluate_keyframes, same model", frame=i)
        assert abs(r64["ssim"] - 1.0) < 1e-12
