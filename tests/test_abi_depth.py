"""CPU tests of gsr_backward_depth's argument validation (no device involved: validation comes first)."""
import ctypes as C

import gs_livm_amd as G


def _call(L, P, dL_ddepth, dL_ddepths):
    one = C.c_void_p(1)  # never dereferenced: validation fails first
    null = C.c_void_p(None)
    #            P  D  M  R  bg   W   H   means shs  col   sc   mod  rot  cov   view proj cam  tanx tany radii
    return L.gsr_backward_depth(P, 0, 1, 0, one, 64, 64, one, one, null, one, 1.0, one, null, one, one, one, 1.0, 1.0, one,
                                one, one, one,           # geometry, binning and image blobs
                                one, one, dL_ddepth,     # dL_dpix, dL_dacc, dL_ddepth
                                *([one] * 9), dL_ddepths, 0, null)


def test_null_depth_pointers_are_refused():
    L = G.lib()
    one, null = C.c_void_p(1), C.c_void_p(None)
    assert _call(L, 5, null, one) == -1 and b"null dL_ddepth" in L.gsr_last_error()
    assert _call(L, 5, one, null) == -1 and b"null dL_ddepths" in L.gsr_last_error()
    assert _call(L, -1, one, one) == -1 and b"bad P" in L.gsr_last_error()


def test_no_gaussians_is_ok():
    L = G.lib()
    null = C.c_void_p(None)
    assert _call(L, 0, null, null) == 0
    assert L.gsr_backward_depth(0, 0, 1, 0, null, 64, 64, *([null] * 4), 1.0, *([null] * 5), 1.0, 1.0, *([null] * 17), 0,
                                null) == 0
