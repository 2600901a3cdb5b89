"""CPU tests of the argument validation of gsr_prune_workspace, gsr_prune_mark and gsr_prune_compact (no device involved:
validation comes first, and nothing is enqueued or written on a refusal)."""
import ctypes as C

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1            # GSR_ERR_INVALID_ARGUMENT
MAX_ROWS = 0x7fffff00   # GSR_PRUNE_MAX_ROWS


def ptr(offset=0):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(4096 + offset)


def _err(L):
    return L.gsr_last_error()


def _mark(L, P=1000, short=0, **over):
    p = dict(xyz=ptr(), scaling=ptr(), rotation=ptr(), opacity=ptr(), drop=NULL, reasons=ptr(), row_map=ptr(),
             counts=ptr(), ws=ptr())
    p.update(over)
    nbytes = max(int(L.gsr_prune_workspace(P)) - short, 0)
    return L.gsr_prune_mark(P, p["xyz"], p["scaling"], p["rotation"], p["opacity"], p["drop"], 1.0 / 255.0, 0.3, 1,
                            p["reasons"], p["row_map"], p["counts"], p["ws"], nbytes, NULL)


def _compact(L, P=1000, widths=(3, 3, 3), src=None, dst=None, reasons=None, row_map=None, n=None, lists=True):
    n = len(widths) if n is None else n
    m = max(len(widths), 1)
    VP = C.c_void_p * m
    src = VP(*(src if src is not None else [ptr().value] * len(widths)))
    dst = VP(*(dst if dst is not None else [ptr(64).value] * len(widths)))
    w = (C.c_int * m)(*widths)
    return L.gsr_prune_compact(P, n, src if lists else None, dst if lists else None, w,
                               ptr() if reasons is None else reasons, ptr() if row_map is None else row_map, NULL)


def test_symbols_and_kernels_are_registered():
    L = G.lib()
    for n in ("gsr_prune_workspace", "gsr_prune_mark", "gsr_prune_compact"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    prune = [k for k in names if k.startswith("k_prune_")]
    assert prune == ["k_prune_mark", "k_prune_scan", "k_prune_rank", "k_prune_compact"]
    # appended behind the last kernel of the evaluation pass: earlier ids keep their place
    assert names.index("k_prune_mark") == names.index("k_pack_depth_u8") + 1
    assert names[-4:] == prune and names.index("k_preprocess") == 0 and names.index("k_model_step") == 27
    assert L.gsr_abi_version() == 2


def test_workspace_is_per_workgroup_not_per_row():
    """Beyond the outputs (reasons, row_map) the scan keeps five int32 per 256 rows: O(P / 256), no per-row scratch."""
    L = G.lib()
    assert L.gsr_prune_workspace(0) == 0 and L.gsr_prune_workspace(-5) == 0 and L.gsr_prune_workspace(MAX_ROWS + 1) == 0
    for P in (1, 255, 256, 257, 4097, 300_007, 2_000_000, MAX_ROWS):
        need = int(L.gsr_prune_workspace(P))
        blocks = (P + 255) // 256
        assert 0 < need <= 20 * blocks + 256, (P, need)
        assert need * 8 < P or P < 4096    # far below one byte per row


def test_mark_refusals_and_their_order():
    L = G.lib()
    for P in (-1, -2 ** 31, MAX_ROWS + 1, 2 ** 31 - 1):
        assert _mark(L, P) == INVALID and b"bad P" in _err(L), P
    for name in ("xyz", "scaling", "rotation", "opacity", "reasons", "row_map", "counts", "ws"):
        assert _mark(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for name in ("xyz", "scaling", "rotation", "opacity", "row_map", "counts", "ws"):
        for off in (1, 2, 3, 5, 6, 7):
            assert _mark(L, **{name: ptr(off)}) == INVALID and b"misaligned" in _err(L), (name, off)
    for P in (1, 256, 257, 300_007):
        need = int(L.gsr_prune_workspace(P))
        assert _mark(L, P, short=1) == INVALID
        assert b"workspace too small" in _err(L) and str(need).encode() in _err(L)
    # the order: shape, then null pointers, then alignment, then the workspace size
    assert _mark(L, -1, xyz=NULL, short=1) == INVALID and b"bad P" in _err(L)
    assert _mark(L, xyz=NULL, scaling=ptr(2), short=1) == INVALID and b"null pointer" in _err(L)
    assert _mark(L, scaling=ptr(2), short=1) == INVALID and b"misaligned" in _err(L)
    # P == 0 needs only the two outputs it writes
    assert _mark(L, 0, row_map=NULL) == INVALID and b"null pointer" in _err(L)
    assert _mark(L, 0, counts=NULL) == INVALID and b"null pointer" in _err(L)


def test_compact_refusals_and_their_order():
    L = G.lib()
    for P in (-1, MAX_ROWS + 1):
        assert _compact(L, P) == INVALID and b"bad P" in _err(L), P
    assert _compact(L, widths=(3,) * 19) == INVALID and b"at most 18" in _err(L)
    assert _compact(L, n=-1) == INVALID and b"tensor count" in _err(L)
    assert _compact(L, widths=(3, -1, 3)) == INVALID and b"bad row width (tensor 1)" in _err(L)
    # one launch holds 2^31 - 1 workgroups of 1024 floats
    assert _compact(L, MAX_ROWS, widths=(64,) * 18) == INVALID and b"too large" in _err(L)
    assert _compact(L, lists=False) == INVALID and b"null pointer" in _err(L)
    assert _compact(L, reasons=NULL) == INVALID and b"null pointer" in _err(L)
    assert _compact(L, row_map=NULL) == INVALID and b"null pointer" in _err(L)
    ok = ptr().value
    assert _compact(L, src=[ok, None, ok]) == INVALID and b"null tensor pointer (tensor 1)" in _err(L)
    assert _compact(L, dst=[ok, ok, None]) == INVALID and b"null tensor pointer (tensor 2)" in _err(L)
    for off in (1, 2, 3, 6):
        assert _compact(L, src=[ok, ptr(off).value, ok]) == INVALID and b"misaligned" in _err(L), off
        assert _compact(L, dst=[ptr(off).value, ok, ok]) == INVALID and b"misaligned" in _err(L), off
        assert _compact(L, row_map=ptr(off)) == INVALID and b"misaligned" in _err(L), off
    # the order: shape, then null pointers, then alignment
    assert _compact(L, -1, src=[None, ok, ok]) == INVALID and b"bad P" in _err(L)
    assert _compact(L, widths=(3, -1, 3), src=[None, ok, ok]) == INVALID and b"bad row width" in _err(L)
    assert _compact(L, src=[ok, None, ok], dst=[ptr(2).value, ok, ok]) == INVALID and b"null tensor pointer" in _err(L)
    # nothing to do is no error and touches nothing: no rows, no tensors, or only tensors of width 0 (whose pointers,
    # like _features_rest's at M = 1, may be null)
    assert _compact(L, 0, src=[None] * 3, dst=[None] * 3, reasons=NULL, row_map=NULL) == 0
    assert _compact(L, widths=(), lists=False, reasons=NULL, row_map=NULL) == 0
    assert _compact(L, widths=(0, 0), src=[None, None], dst=[None, None]) == 0
