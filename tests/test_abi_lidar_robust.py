"""CPU tests of the argument validation of gsr_lidar_occlusion_filter and gsr_lidar_depth_loss_robust (no device
involved: validation comes first)."""
import ctypes as C
import math

import torch

import gs_livm_amd as G

ONE = C.c_void_p(1)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
INF = float("inf")
BASE = 1 << 20        # a made-up device address for the overlap tests


def _filter(L, H=16, W=16, src=C.c_void_p(BASE), dst=C.c_void_p(BASE + (1 << 16)), radius=1, tol=0.05, counts=NULL):
    return L.gsr_lidar_occlusion_filter(H, W, src, radius, tol, dst, counts, NULL)


def _loss(L, H=16, W=16, ptrs=None, acc_min=0.5, short=0, ws=ONE, huber_abs=0.1, huber_rel=0.01, clip_abs=0.25,
          clip_rel=0.01):
    p = dict(depth=ONE, acc=ONE, lidar=ONE, out4=ONE, g_depth=NULL, g_acc=NULL)
    p.update(ptrs or {})
    nbytes = max(int(L.gsr_lidar_depth_loss_robust_workspace(H, W)) - short, 0)
    return L.gsr_lidar_depth_loss_robust(H, W, p["depth"], p["acc"], p["lidar"], acc_min, 1.0, huber_abs, huber_rel,
                                         clip_abs, clip_rel, p["out4"], p["g_depth"], p["g_acc"], ws, nbytes, NULL)


def test_symbols_are_exported():
    for s in ("gsr_lidar_occlusion_filter", "gsr_lidar_depth_loss_robust", "gsr_lidar_depth_loss_robust_workspace"):
        assert s in G._capi.EXPORTS and hasattr(G.lib(), s)
    # no profiler id was added: the mask has 64 bits and the new kernels are timed under the existing LiDAR ids
    names = [G.lib().gsr_kernel_name(i).decode() for i in range(G.lib().gsr_kernel_count())]
    assert len(set(names)) == len(names) <= 64
    assert G.lib().gsr_abi_version() == 2
    assert callable(G.lidar_occlusion_filter) and issubclass(G.RobustLidarDepthLoss, torch.autograd.Function)
    for name in ("lidar_occlusion_filter", "RobustLidarDepthLoss"):
        assert name in G.__all__


def test_filter_refusals():
    L = G.lib()
    err = L.gsr_last_error
    for H, W in ((0, 16), (16, 0), (-3, 16), (16, -3)):
        assert _filter(L, H=H, W=W) == -1 and b"bad image shape" in err(), (H, W)
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert _filter(L, H=H, W=W, dst=C.c_void_p(1 << 40)) == -1 and b"too large" in err(), (H, W)
    assert _filter(L, src=NULL) == -1 and b"null pointer" in err()
    assert _filter(L, dst=NULL) == -1 and b"null pointer" in err()
    for r in (-1, 4, 100, -(1 << 31)):
        assert _filter(L, radius=r) == -1 and b"bad radius" in err(), r
    for t in (-0.01, INF, -INF, math.nan):
        assert _filter(L, tol=t) == -1 and b"bad tol" in err(), t
    # filtered == lidar_depth, partial overlaps from either side down to a single byte
    n = 16 * 16 * 4
    for d in (0, 4, n - 4, n - 1, -4, -(n - 4), -(n - 1)):
        assert _filter(L, dst=C.c_void_p(BASE + d)) == -1 and b"overlap" in err(), d
    # the order: the shape, the pointers, radius, tol, the overlap
    assert _filter(L, H=0, src=NULL, radius=9) == -1 and b"bad image shape" in err()
    assert _filter(L, src=NULL, radius=9) == -1 and b"null pointer" in err()
    assert _filter(L, radius=9, tol=-1.0) == -1 and b"bad radius" in err()
    assert _filter(L, tol=-1.0, dst=C.c_void_p(BASE)) == -1 and b"bad tol" in err()


def test_loss_bad_shapes_are_refused():
    L = G.lib()
    for H, W in ((0, 16), (16, 0), (0, 0), (-3, 16), (16, -3)):
        assert _loss(L, H, W) == -1 and b"bad image shape" in L.gsr_last_error(), (H, W)
        assert L.gsr_lidar_depth_loss_robust_workspace(H, W) == 0
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert _loss(L, H, W) == -1 and b"too large" in L.gsr_last_error(), (H, W)
        assert L.gsr_lidar_depth_loss_robust_workspace(H, W) == 0
    assert L.gsr_lidar_depth_loss_robust_workspace(1, 1) > 0 and L.gsr_lidar_depth_loss_robust_workspace(46340, 46340) > 0


def test_loss_null_pointers_and_parameters_are_refused():
    L = G.lib()
    err = L.gsr_last_error
    for name in ("depth", "acc", "lidar", "out4"):
        assert _loss(L, ptrs={name: NULL}) == -1 and b"null pointer" in err(), name
    assert _loss(L, ws=NULL) == -1 and b"null pointer" in err()
    for a in (0.0, -0.5, INF, math.nan):
        assert _loss(L, acc_min=a) == -1 and b"bad acc_min" in err(), a
    for name in ("huber_abs", "huber_rel", "clip_rel"):
        for v in (-0.01, math.nan, INF, -INF):
            assert _loss(L, **{name: v}) == -1 and ("bad " + name).encode() in err(), (name, v)
    for v in (-0.01, math.nan, -INF):
        assert _loss(L, clip_abs=v) == -1 and b"bad clip_abs" in err(), v
    # the order: the shape, the pointers, acc_min, the four parameters in the order of the signature, the workspace
    assert _loss(L, 0, 0, ptrs={"depth": NULL}, ws=NULL) == -1 and b"bad image shape" in err()
    assert _loss(L, ptrs={"depth": NULL}, acc_min=0.0) == -1 and b"null pointer" in err()
    assert _loss(L, acc_min=0.0, huber_abs=-1.0) == -1 and b"bad acc_min" in err()
    assert _loss(L, huber_abs=-1.0, huber_rel=-1.0) == -1 and b"bad huber_abs" in err()
    assert _loss(L, huber_rel=-1.0, clip_abs=-1.0) == -1 and b"bad huber_rel" in err()
    assert _loss(L, clip_abs=-1.0, clip_rel=-1.0) == -1 and b"bad clip_abs" in err()
    assert _loss(L, clip_rel=-1.0, short=1) == -1 and b"bad clip_rel" in err()


def test_loss_short_workspace_is_refused():
    L = G.lib()
    for H, W in ((1, 1), (37, 61), (512, 640)):
        need = int(L.gsr_lidar_depth_loss_robust_workspace(H, W))
        assert _loss(L, H, W, short=1) == -1
        msg = L.gsr_last_error()
        assert b"workspace too small" in msg and str(need).encode() in msg
        # nothing is stored per pixel: 24 bytes (two doubles and two ints) per workgroup of 256 pixels, one float, and
        # the alignment of five carvings and of the caller's pointer
        blocks = (H * W + 255) // 256
        assert 24 * blocks + 4 <= need <= 24 * blocks + 4 + 6 * 256
        assert need <= H * W // 8 + 1600                   # i.e. under an eighth of a byte per pixel
    # +inf for clip_abs and zeros everywhere else (the identity parameters) pass validation: only the workspace is short
    assert _loss(L, huber_abs=0.0, huber_rel=0.0, clip_abs=INF, clip_rel=0.0, short=1) == -1
    assert b"workspace too small" in L.gsr_last_error()
