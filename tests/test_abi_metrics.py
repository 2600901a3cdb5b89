"""CPU tests of the argument validation of gsr_image_metrics, gsr_pack_image_u8 and gsr_pack_depth_u8 (no device
involved: validation comes first, and nothing is enqueued or written on a refusal)."""
import ctypes as C
import math

import gs_livm_amd as G

ONE = C.c_void_p(1)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
WIN = (C.c_float * 11)(*([1.0 / 11.0] * 11))
INVALID = -1          # GSR_ERR_INVALID_ARGUMENT
TOO_LARGE = ((65536, 32768), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (46341, 46341))   # H W >= 2^31 - 1


def _metrics(L, Cn=3, H=16, W=16, ptrs=None, win=WIN, short=0):
    p = dict(img=ONE, gt=ONE, out4=ONE, totals=NULL, ws=ONE)
    p.update(ptrs or {})
    nbytes = max(int(L.gsr_image_metrics_workspace(Cn, H, W)) - short, 0)
    return L.gsr_image_metrics(Cn, H, W, p["img"], p["gt"], win, p["out4"], p["totals"], p["ws"], nbytes, NULL)


def _err(L):
    return L.gsr_last_error()


def test_symbols_and_kernels_are_registered():
    L = G.lib()
    for n in ("gsr_image_metrics", "gsr_image_metrics_workspace", "gsr_pack_image_u8", "gsr_pack_depth_u8"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    for k in ("k_metrics_forward", "k_metrics_finalize", "k_pack_image_u8", "k_pack_depth_u8"):
        assert k in names
    assert names.index("k_delta_convert") < names.index("k_metrics_forward")   # appended: earlier ids keep their place
    assert L.gsr_abi_version() == 2


def test_metrics_refusals_and_their_order():
    L = G.lib()
    for shape in ((0, 16, 16), (3, 0, 16), (3, 16, 0), (-1, 16, 16), (3, -2, 16), (3, 16, -2)):
        assert _metrics(L, *shape) == INVALID and b"bad image shape" in _err(L), shape
        assert L.gsr_image_metrics_workspace(*shape) == 0
    for H, W in TOO_LARGE:
        assert H * W >= 2 ** 31 - 1
        assert _metrics(L, 1, H, W) == INVALID and b"too large" in _err(L), (H, W)
        assert L.gsr_image_metrics_workspace(1, H, W) == 0
    assert L.gsr_image_metrics_workspace(1, 46340, 46340) > 0 and L.gsr_image_metrics_workspace(1, 1, 2 ** 31 - 2) > 0
    for name in ("img", "gt", "out4", "ws"):
        assert _metrics(L, ptrs={name: NULL}) == INVALID and b"null pointer" in _err(L), name
    assert _metrics(L, win=None) == INVALID and b"null pointer" in _err(L)
    for shape in ((3, 16, 16), (1, 1, 1), (3, 512, 640)):
        need = int(L.gsr_image_metrics_workspace(*shape))
        assert _metrics(L, *shape, short=1) == INVALID
        assert b"workspace too small" in _err(L) and str(need).encode() in _err(L)
    # the order: shape, then size, then null pointers, then the workspace
    assert _metrics(L, 0, 2 ** 20, 2 ** 20, ptrs={"img": NULL}) == INVALID and b"bad image shape" in _err(L)
    assert _metrics(L, 1, 2 ** 20, 2 ** 20, ptrs={"img": NULL}) == INVALID and b"too large" in _err(L)
    assert _metrics(L, ptrs={"img": NULL}, short=1) == INVALID and b"null pointer" in _err(L)


def test_metrics_workspace_holds_partials_only():
    """At most 16 bytes per 54 x 32 work unit and a little bookkeeping: no per-pixel map is allocated (the photometric
    loss asks for 36 bytes per pixel-channel)."""
    L = G.lib()
    for Cn, H, W in ((3, 1080, 1920), (3, 512, 640), (1, 1, 1)):
        units = Cn * math.ceil(H / 32) * math.ceil(W / 54)
        need = int(L.gsr_image_metrics_workspace(Cn, H, W))
        assert 0 < need <= 16 * units + 4096, (Cn, H, W, need)
        assert need < int(L.gsr_photometric_loss_workspace(Cn, H, W)) // 100 or H * W == 1


def _image(L, H=8, W=8, img=ONE, out=ONE, pitch=None, bgr=1):
    return L.gsr_pack_image_u8(H, W, img, bgr, out, 3 * W if pitch is None else pitch, NULL)


def _depth(L, H=8, W=8, depth=ONE, out=ONE, pitch=None, max_depth=50.0):
    return L.gsr_pack_depth_u8(H, W, depth, max_depth, out, W if pitch is None else pitch, NULL)


def test_pack_refusals_and_their_order():
    L = G.lib()
    for call in (_image, _depth):
        for H, W in ((0, 8), (8, 0), (-1, 8), (8, -1)):
            assert call(L, H, W) == INVALID and b"bad image shape" in _err(L), (call.__name__, H, W)
        for H, W in TOO_LARGE:
            assert call(L, H, W) == INVALID and b"too large" in _err(L), (call.__name__, H, W)
        assert call(L, out=NULL) == INVALID and b"null pointer" in _err(L)
    assert _image(L, img=NULL) == INVALID and b"null pointer" in _err(L)
    assert _depth(L, depth=NULL) == INVALID and b"null pointer" in _err(L)
    assert _image(L, pitch=23) == INVALID and b"pitch too small" in _err(L) and b"24" in _err(L)
    assert _image(L, pitch=0) == INVALID and b"pitch too small" in _err(L)
    assert _depth(L, pitch=7) == INVALID and b"pitch too small" in _err(L) and b"8" in _err(L)
    for bad in (0.0, -0.0, -50.0, math.inf, -math.inf, math.nan):
        assert _depth(L, max_depth=bad) == INVALID and b"max_depth" in _err(L), bad
    # the order: shape, size, null pointers, pitch, max_depth
    assert _image(L, 0, 8, img=NULL, pitch=0) == INVALID and b"bad image shape" in _err(L)
    assert _image(L, 2 ** 20, 2 ** 20, img=NULL, pitch=0) == INVALID and b"too large" in _err(L)
    assert _image(L, img=NULL, pitch=0) == INVALID and b"null pointer" in _err(L)
    assert _depth(L, depth=NULL, pitch=0, max_depth=0.0) == INVALID and b"null pointer" in _err(L)
    assert _depth(L, pitch=0, max_depth=0.0) == INVALID and b"pitch too small" in _err(L)
