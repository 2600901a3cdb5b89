"""CPU tests of the argument validation of gsr_lidar_depth_image and gsr_lidar_depth_loss (no device involved:
validation comes first)."""
import ctypes as C
import math

import gs_livm_amd as G

ONE = C.c_void_p(1)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
F9 = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
F12 = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
INF = float("inf")


def _image(L, n=5, H=16, W=16, points=ONE, T=F12, K=F9, lo=0.2, hi=INF, image=ONE, counts=NULL):
    return L.gsr_lidar_depth_image(n, points, T, K, H, W, lo, hi, image, counts, NULL)


def _loss(L, H=16, W=16, ptrs=None, acc_min=0.5, short=0, ws=ONE):
    p = dict(depth=ONE, acc=ONE, lidar=ONE, out3=ONE, g_depth=NULL, g_acc=NULL)
    p.update(ptrs or {})
    nbytes = max(int(L.gsr_lidar_depth_loss_workspace(H, W)) - short, 0)
    return L.gsr_lidar_depth_loss(H, W, p["depth"], p["acc"], p["lidar"], acc_min, 1.0, p["out3"], p["g_depth"],
                                  p["g_acc"], ws, nbytes, NULL)


def test_symbols_are_exported():
    for s in ("gsr_lidar_depth_image", "gsr_lidar_depth_loss", "gsr_lidar_depth_loss_workspace"):
        assert s in G._capi.EXPORTS and hasattr(G.lib(), s)
    names = [G.lib().gsr_kernel_name(i).decode() for i in range(G.lib().gsr_kernel_count())]
    for k in ("k_lidar_clear", "k_lidar_splat", "k_lidar_convert", "k_lidar_loss_forward", "k_lidar_loss_finish",
              "k_lidar_loss_grads"):
        assert k in names
    assert len(set(names)) == len(names) <= 64        # (the profiler's mask has 64 bits)
    assert G.lib().gsr_abi_version() == 2


def test_image_refusals():
    L = G.lib()
    err = L.gsr_last_error
    assert _image(L, n=-1) == -1 and b"bad n" in err()
    for H, W in ((0, 16), (16, 0), (-3, 16), (16, -3)):
        assert _image(L, H=H, W=W) == -1 and b"bad image shape" in err(), (H, W)
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert H * W >= 2 ** 31
        assert _image(L, H=H, W=W) == -1 and b"too large" in err(), (H, W)
    assert _image(L, points=NULL) == -1 and b"null pointer" in err()
    assert _image(L, T=None) == -1 and b"null pointer" in err()
    assert _image(L, K=None) == -1 and b"null pointer" in err()
    assert _image(L, image=NULL) == -1 and b"null pointer" in err()
    for lo in (-0.1, INF, math.nan):
        assert _image(L, lo=lo) == -1 and b"bad min_depth" in err(), lo
    for lo, hi in ((0.2, 0.2), (0.2, 0.1), (0.0, 0.0), (0.2, math.nan), (0.2, -INF)):
        assert _image(L, lo=lo, hi=hi) == -1 and b"bad max_depth" in err(), (lo, hi)
    # the order: n, the shape, then the pointers, then the depths
    assert _image(L, n=-1, H=0, points=NULL) == -1 and b"bad n" in err()
    assert _image(L, H=0, points=NULL, lo=-1.0) == -1 and b"bad image shape" in err()
    assert _image(L, image=NULL, lo=-1.0) == -1 and b"null pointer" in err()


def test_loss_bad_shapes_are_refused():
    L = G.lib()
    for H, W in ((0, 16), (16, 0), (0, 0), (-3, 16), (16, -3)):
        assert _loss(L, H, W) == -1 and b"bad image shape" in L.gsr_last_error(), (H, W)
        assert L.gsr_lidar_depth_loss_workspace(H, W) == 0
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert _loss(L, H, W) == -1 and b"too large" in L.gsr_last_error(), (H, W)
        assert L.gsr_lidar_depth_loss_workspace(H, W) == 0
    assert L.gsr_lidar_depth_loss_workspace(1, 1) > 0 and L.gsr_lidar_depth_loss_workspace(46340, 46340) > 0


def test_loss_null_pointers_and_acc_min_are_refused():
    L = G.lib()
    for name in ("depth", "acc", "lidar", "out3"):
        assert _loss(L, ptrs={name: NULL}) == -1 and b"null pointer" in L.gsr_last_error(), name
    assert _loss(L, ws=NULL) == -1 and b"null pointer" in L.gsr_last_error()
    for a in (0.0, -0.5, INF, math.nan):
        assert _loss(L, acc_min=a) == -1 and b"bad acc_min" in L.gsr_last_error(), a
    # the order: the shape, the pointers, acc_min, the workspace
    assert _loss(L, 0, 0, ptrs={"depth": NULL}, ws=NULL) == -1 and b"bad image shape" in L.gsr_last_error()
    assert _loss(L, ptrs={"depth": NULL}, acc_min=0.0) == -1 and b"null pointer" in L.gsr_last_error()
    assert _loss(L, acc_min=0.0, short=1) == -1 and b"bad acc_min" in L.gsr_last_error()


def test_loss_short_workspace_is_refused():
    L = G.lib()
    for H, W in ((1, 1), (37, 61), (512, 640)):
        need = int(L.gsr_lidar_depth_loss_workspace(H, W))
        assert _loss(L, H, W, short=1) == -1
        msg = L.gsr_last_error()
        assert b"workspace too small" in msg and str(need).encode() in msg
        # nothing is stored per pixel: 12 bytes (a double and an int) per workgroup of 256 pixels, one float, and
        # the alignment of three carvings and of the caller's pointer
        blocks = (H * W + 255) // 256
        assert 12 * blocks + 4 <= need <= 12 * blocks + 4 + 4 * 256
        assert need <= H * W // 16 + 1040                  # i.e. under a sixteenth of a byte per pixel
