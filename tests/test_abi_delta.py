"""CPU tests of gsr_delta_depth_loss's argument validation (no device involved: validation comes first)."""
import ctypes as C

import gs_livm_amd as G

ONE = C.c_void_p(1)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
F9 = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
F12 = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _call(L, H=16, W=16, ptrs=None, host=None, short=0, ws=ONE):
    """ptrs: overrides of the device pointers by name; host: overrides of the three host matrices."""
    p = dict(depth_src=ONE, acc_src=ONE, depth_ref=ONE, acc_ref=ONE, out3=ONE, warped=NULL, g_src=NULL, g_ref=NULL)
    p.update(ptrs or {})
    h = dict(inv_K=F9, K=F9, T=F12)
    h.update(host or {})
    nbytes = max(int(L.gsr_delta_depth_loss_workspace(H, W)) - short, 0)
    return L.gsr_delta_depth_loss(H, W, p["depth_src"], p["acc_src"], p["depth_ref"], p["acc_ref"], h["inv_K"], h["K"],
                                  h["T"], 0.2, p["out3"], p["warped"], p["g_src"], p["g_ref"], ws, nbytes, NULL)


def test_symbols_are_exported():
    assert "gsr_delta_depth_loss" in G._capi.EXPORTS and "gsr_delta_depth_loss_workspace" in G._capi.EXPORTS
    names = [G.lib().gsr_kernel_name(i).decode() for i in range(G.lib().gsr_kernel_count())]
    for k in ("k_delta_project", "k_delta_sample", "k_delta_scatter", "k_delta_convert"):
        assert k in names


def test_bad_shapes_are_refused():
    L = G.lib()
    for H, W in ((1, 16), (16, 1), (0, 0), (-3, 16), (16, -3), (1, 1)):
        assert _call(L, H, W) == -1 and b"bad image shape" in L.gsr_last_error(), (H, W)
        assert L.gsr_delta_depth_loss_workspace(H, W) == 0
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert H * W >= 2 ** 31
        assert _call(L, H, W) == -1 and b"too large" in L.gsr_last_error(), (H, W)
        assert L.gsr_delta_depth_loss_workspace(H, W) == 0
    assert L.gsr_delta_depth_loss_workspace(2, 2) > 0 and L.gsr_delta_depth_loss_workspace(46340, 46340) > 0


def test_null_required_pointers_are_refused():
    L = G.lib()
    for name in ("depth_src", "acc_src", "depth_ref", "acc_ref", "out3"):
        assert _call(L, ptrs={name: NULL}) == -1 and b"null pointer" in L.gsr_last_error(), name
    for name in ("inv_K", "K", "T"):
        assert _call(L, host={name: None}) == -1 and b"null pointer" in L.gsr_last_error(), name
    assert _call(L, ws=NULL) == -1 and b"null pointer" in L.gsr_last_error()


def test_short_workspace_is_refused():
    L = G.lib()
    for H, W in ((2, 2), (37, 61), (512, 640)):
        need = int(L.gsr_delta_depth_loss_workspace(H, W))
        assert _call(L, H, W, short=1) == -1
        msg = L.gsr_last_error()
        assert b"workspace too small" in msg and str(need).encode() in msg
        # 28 bytes per pixel of scratch and a little bookkeeping, whatever the alignment of the caller's pointer
        assert 28 * H * W <= need <= 28 * H * W + 16 * (H * W // 256 + 1) + 4096


def test_validation_order_shape_before_pointers():
    L = G.lib()
    assert _call(L, 1, 1, ptrs={"depth_src": NULL}, ws=NULL) == -1 and b"bad image shape" in L.gsr_last_error()
