"""CPU tests of the argument validation of the contribution entry points (gsr_contribution_workspace, gsr_contribution,
gsr_contribution_finish): no device involved -- validation comes first, and nothing is enqueued or written on a refusal --
and of what the feature registers (symbols, no new profiler id, Python names)."""
import ctypes as C

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1                  # GSR_ERR_INVALID_ARGUMENT


def ptr(offset=0, base=1 << 20):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(base + offset)


def _err(L):
    return L.gsr_last_error()


def _walk(L, P=1000, R=5000, W=640, H=480, geom=ptr(), binning=ptr(0, 2 << 20), image=ptr(0, 3 << 20),
          rows=ptr(0, 4 << 20)):
    return L.gsr_contribution(P, R, W, H, geom, binning, image, rows, NULL)


def _finish(L, P=1000, rows=ptr(), min_pixels=1, min_weight=0.0, n_touched=ptr(0, 2 << 20), weight_sum=ptr(0, 3 << 20),
            weight_max=ptr(0, 4 << 20), mask=ptr(0, 5 << 20), stats=ptr(0, 6 << 20)):
    return L.gsr_contribution_finish(P, rows, min_pixels, min_weight, n_touched, weight_sum, weight_max, mask, stats, NULL)


def test_symbols_python_names_and_no_new_kernel_id():
    L = G.lib()
    for n in ("gsr_contribution_workspace", "gsr_contribution", "gsr_contribution_finish"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    # the profiler word is full: the new kernels are timed under k_visibility and no id was added
    assert L.gsr_kernel_count() == 64 and len(set(names)) == 64 and not [k for k in names if "contrib" in k]
    assert L.gsr_abi_version() == 2
    for n in ("Contribution", "contribution", "render_contribution", "low_contribution"):
        assert n in G.__all__ and hasattr(G, n), n
    for n in ("enable_contribution_stats", "contribution_stats", "reset_contribution_stats"):
        assert hasattr(G.GrowableGaussians, n), n
    for n in ("contribution_rows", "contribution_finish"):
        assert hasattr(G._capi, n), n
    assert G.Contribution._fields == ("n_touched", "weight_sum", "weight_max", "mask", "rows")


def test_workspace_is_sixteen_bytes_a_row():
    L = G.lib()
    for P, want in ((0, 0), (-1, 0), (-2 ** 31, 0), (1, 16), (1000, 16_000), (2 ** 31 - 1, 16 * (2 ** 31 - 1))):
        assert L.gsr_contribution_workspace(P) == want, P


def test_contribution_refusals_and_their_order():
    L = G.lib()
    for kw in (dict(P=-1), dict(R=-1), dict(W=0), dict(W=-5), dict(H=0), dict(H=-2 ** 31)):
        assert _walk(L, **kw) == INVALID and b"bad P/R/width/height" in _err(L), kw
    for W, H in ((65536, 32768), (2 ** 31 - 1, 2), (46341, 46341)):      # W * H >= 2^31
        assert _walk(L, W=W, H=H) == INVALID and b"image plane too large" in _err(L), (W, H)
    assert _walk(L, rows=NULL) == INVALID and b"null pointer" in _err(L)
    for name in ("geom", "binning", "image"):
        assert _walk(L, **{name: NULL}) == INVALID and b"null state blob" in _err(L), name
    for off in (1, 2, 3, 4, 5, 6, 7, 12):
        assert _walk(L, rows=ptr(off, 4 << 20)) == INVALID and b"8-byte" in _err(L), off
    # the order: shape (counts, then the plane), null pointers (rows, then blobs), alignment
    assert _walk(L, P=-1, W=65536, H=32768, rows=NULL) == INVALID and b"bad P/R" in _err(L)
    assert _walk(L, W=65536, H=32768, rows=NULL) == INVALID and b"plane too large" in _err(L)
    assert _walk(L, rows=NULL, geom=NULL) == INVALID and b"null pointer" in _err(L)
    assert _walk(L, rows=ptr(4), geom=NULL) == INVALID and b"null state blob" in _err(L)
    # P == 0 is legal whatever the pointers: nothing to write, nothing enqueued
    assert _walk(L, P=0, R=0, geom=NULL, binning=NULL, image=NULL, rows=NULL) == 0 and _err(L) == b""
    assert _walk(L, P=0, rows=ptr(3)) == 0
    # ... but a bad shape is refused first
    assert _walk(L, P=0, W=0) == INVALID and _walk(L, P=0, W=65536, H=32768) == INVALID


def test_finish_refusals_and_their_order():
    L = G.lib()
    none = dict(n_touched=NULL, weight_sum=NULL, weight_max=NULL, mask=NULL, stats=NULL)
    assert _finish(L, P=-1) == INVALID and b"bad P" in _err(L)
    assert _finish(L, min_pixels=-1) == INVALID and b"bad min_pixels" in _err(L)
    for w in (-1e-9, float("nan"), -float("inf")):
        assert _finish(L, min_weight=w) == INVALID and b"bad min_weight" in _err(L), w
    assert _finish(L, **none) == INVALID and b"no output is asked for" in _err(L)
    assert _finish(L, rows=NULL) == INVALID and b"null pointer" in _err(L)
    for off in (1, 2, 4, 7, 12):
        assert _finish(L, rows=ptr(off)) == INVALID and b"8-byte" in _err(L), off
    for name in ("n_touched", "weight_sum", "weight_max", "stats"):
        for off in (1, 2, 3):
            assert _finish(L, **{name: ptr(off, 7 << 20)}) == INVALID and b"4-byte" in _err(L), (name, off)
    # the order: shape, nothing asked for, null pointers, alignment (the rows first)
    assert _finish(L, P=-1, min_pixels=-1, rows=NULL, **none) == INVALID and b"bad P" in _err(L)
    assert _finish(L, min_pixels=-1, min_weight=-1.0, rows=NULL, **none) == INVALID and b"bad min_pixels" in _err(L)
    assert _finish(L, min_weight=-1.0, rows=NULL, **none) == INVALID and b"bad min_weight" in _err(L)
    assert _finish(L, rows=NULL, **none) == INVALID and b"no output" in _err(L)
    assert _finish(L, rows=NULL, n_touched=ptr(2)) == INVALID and b"null pointer" in _err(L)
    assert _finish(L, rows=ptr(4), n_touched=ptr(2)) == INVALID and b"8-byte" in _err(L)
    # P == 0 with an output asked for is legal; with none it is refused like any other P
    assert _finish(L, P=0, rows=NULL) == 0 and _err(L) == b""
    assert _finish(L, P=0, rows=NULL, **none) == INVALID and b"no output" in _err(L)
