"""CPU tests of the validation that gsr_forward, gsr_backward and gsr_backward_depth share (no device involved: the
pointers are never dereferenced, validation fails first): the alignment of `rotations` (include/gsraster.h), the
(D, M) rule and the "scales + rotations or a precomputed covariance" rule, which the backwards did not check."""
import ctypes as C

import pytest

import gs_livm_amd as G

NULL = C.c_void_p(None)
BASE = 0x1000   # 16-byte aligned, never dereferenced


def _p(off=0):
    return C.c_void_p(BASE + off)


def _forward(L, P=5, D=0, M=1, scales=None, rot=None, cov=NULL, colors=NULL):
    noop = G._capi.ALLOC_FN(lambda ctx, n: None)
    one = _p()
    return L.gsr_forward(noop, None, noop, None, noop, None, P, D, M, one, 64, 64, one, one, colors, one,
                         one if scales is None else scales, 1.0, one if rot is None else rot, cov, one, one, one, 1.0,
                         1.0, 0, one, one, one, NULL, 0, NULL)


def _backward(L, depth, P=5, D=0, M=1, scales=None, rot=None, cov=NULL, colors=NULL):
    one = _p()
    head = (P, D, M, 0, one, 64, 64, one, one, colors, one if scales is None else scales, 1.0,
            one if rot is None else rot, cov, one, one, one, 1.0, 1.0, one, one, one, one, one, one)
    if depth:
        return L.gsr_backward_depth(*head, one, *([one] * 9), one, 0, NULL)
    return L.gsr_backward(*head, *([one] * 9), 0, NULL)


ENTRIES = ("gsr_forward", "gsr_backward", "gsr_backward_depth")


def _call(L, entry, **kw):
    if entry == "gsr_forward":
        return _forward(L, **kw)
    return _backward(L, entry == "gsr_backward_depth", **kw)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("off", [4, 8, 12])
def test_misaligned_rotations_is_refused(entry, off):
    L = G.lib()
    assert _call(L, entry, rot=_p(off)) == -1 and b"rotations" in L.gsr_last_error()
    assert b"16-byte" in L.gsr_last_error()
    # not read when the covariance is precomputed: no alignment asked of it (the forward then goes on to its allocators,
    # which return NULL here; the backwards would go on to the device, so only the forward is called)
    if entry == "gsr_forward":
        assert _call(L, entry, rot=_p(off), cov=_p()) == -2 and b"allocator" in L.gsr_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("D,M", [(3, 4), (0, 17), (4, 16), (1, 2), (-1, 1)])
def test_illegal_degree_and_coefficient_count_are_refused(entry, D, M):
    L = G.lib()
    assert _call(L, entry, D=D, M=M) == -4 and b"SH degree" in L.gsr_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_scales_without_rotations_is_refused(entry):
    L = G.lib()
    assert _call(L, entry, rot=NULL) == -1 and b"scales+rotations" in L.gsr_last_error()
    assert _call(L, entry, scales=NULL) == -1 and b"scales+rotations" in L.gsr_last_error()


@pytest.mark.parametrize("depth", [False, True])
def test_no_gaussians_stays_ok(depth):
    """An aligned, legal call with P = 0 is GSR_OK (the forward's P = 0 zero-fills its images: a device call, tested
    in test_gpu_parity.py::test_empty_input_is_a_noop)."""
    L = G.lib()
    assert _backward(L, depth, P=0) == 0
    assert _backward(L, depth, P=0, D=1, M=9) == 0


def test_the_degree_rule_is_not_applied_to_precomputed_colours():
    """As in the forward: D and M are not read when the colours are precomputed."""
    L = G.lib()
    assert _forward(L, D=4, M=0, colors=_p()) == -2 and b"allocator" in L.gsr_last_error()
