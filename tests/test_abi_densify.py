"""CPU tests of the argument validation of gsr_density_accumulate, gsr_densify_workspace, gsr_densify_mark and
gsr_densify_apply (no device involved: validation comes first, and nothing is enqueued or written on a refusal)."""
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


def _accumulate(L, P=1000, **over):
    p = dict(radii=ptr(), grad=ptr(), stats=ptr())
    p.update(over)
    return L.gsr_density_accumulate(P, p["radii"], p["grad"], p["stats"], NULL)


def _mark(L, P=1000, short=0, **over):
    p = dict(stats=ptr(), scaling=ptr(), kinds=ptr(), offsets=ptr(), counts=ptr(), ws=ptr())
    p.update(over)
    nbytes = max(int(L.gsr_densify_workspace(P)) - short, 0)
    return L.gsr_densify_mark(P, p["stats"], p["scaling"], 0.0002, 0.01, -1, p["kinds"], p["offsets"], p["counts"],
                              p["ws"], nbytes, NULL)


LEAVES = ("xyz", "fdc", "frest", "scaling", "rotation", "opacity")


def _apply(L, P=1000, M=4, n_new=10, m="all", v="all", **over):
    p = dict(kinds=ptr(), offsets=ptr(), stats=ptr())
    p.update({n: ptr() for n in LEAVES})
    p.update(over)
    VP = C.c_void_p * 6
    arr = lambda a: None if a is None else VP(*([ptr().value] * 6 if a == "all" else a))  # noqa: E731
    return L.gsr_densify_apply(P, M, n_new, p["kinds"], p["offsets"], 7, *[p[n] for n in LEAVES], arr(m), arr(v),
                               p["stats"], NULL)


def test_symbols_and_kernels_are_registered():
    L = G.lib()
    for n in ("gsr_density_accumulate", "gsr_densify_workspace", "gsr_densify_mark", "gsr_densify_apply"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    new = ["k_density_accumulate", "k_densify_mark", "k_densify_scan", "k_densify_rank", "k_densify_apply"]
    at = names.index("k_lidar_loss_grads") + 1                  # directly behind the LiDAR depth term
    assert names[at:at + 5] == new
    assert names[-4:] == ["k_prune_mark", "k_prune_scan", "k_prune_rank", "k_prune_compact"]
    assert names.index("k_prune_mark") == names.index("k_pack_depth_u8") + 1
    assert names.index("k_preprocess") == 0 and names.index("k_model_step") == 27
    assert len(set(names)) == len(names) <= 64                  # the profiler's mask has 64 bits
    assert L.gsr_abi_version() == 2


def test_workspace_is_per_workgroup_not_per_row():
    L = G.lib()
    assert L.gsr_densify_workspace(0) == 0 and L.gsr_densify_workspace(-5) == 0
    assert L.gsr_densify_workspace(MAX_ROWS + 1) == 0
    for P in (1, 255, 256, 257, 4097, 262_144 + 257, 2_000_000, MAX_ROWS):
        need = int(L.gsr_densify_workspace(P))
        blocks = (P + 255) // 256
        assert 0 < need <= 8 * blocks + 256, (P, need)
        assert need * 16 < P or P < 4096    # far below one byte per row


def test_accumulate_refusals_and_their_order():
    L = G.lib()
    for P in (-1, -2 ** 31, MAX_ROWS + 1, 2 ** 31 - 1):
        assert _accumulate(L, P) == INVALID and b"bad P" in _err(L), P
    for name in ("radii", "grad", "stats"):
        assert _accumulate(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
        for off in (1, 2, 3, 5, 6, 7):
            assert _accumulate(L, **{name: ptr(off)}) == INVALID and b"misaligned" in _err(L), (name, off)
    assert _accumulate(L, -1, radii=NULL) == INVALID and b"bad P" in _err(L)
    assert _accumulate(L, radii=NULL, grad=ptr(2)) == INVALID and b"null pointer" in _err(L)
    assert _accumulate(L, 0, radii=NULL, grad=NULL, stats=NULL) == 0      # no rows: touches nothing


def test_mark_refusals_and_their_order():
    L = G.lib()
    for P in (-1, -2 ** 31, MAX_ROWS + 1, 2 ** 31 - 1):
        assert _mark(L, P) == INVALID and b"bad P" in _err(L), P
    for name in ("stats", "scaling", "kinds", "offsets", "counts", "ws"):
        assert _mark(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for name in ("stats", "scaling", "offsets", "counts", "ws"):
        for off in (1, 2, 3, 5, 6, 7):
            assert _mark(L, **{name: ptr(off)}) == INVALID and b"misaligned" in _err(L), (name, off)
    for P in (1, 256, 257, 300_007):
        need = int(L.gsr_densify_workspace(P))
        assert _mark(L, P, short=1) == INVALID
        assert b"workspace too small" in _err(L) and str(need).encode() in _err(L)
    # the order: shape, then null pointers, then alignment, then the workspace size
    assert _mark(L, -1, stats=NULL, short=1) == INVALID and b"bad P" in _err(L)
    assert _mark(L, stats=NULL, scaling=ptr(2), short=1) == INVALID and b"null pointer" in _err(L)
    assert _mark(L, scaling=ptr(2), short=1) == INVALID and b"misaligned" in _err(L)
    # P == 0 needs only the two outputs it writes
    assert _mark(L, 0, offsets=NULL) == INVALID and b"null pointer" in _err(L)
    assert _mark(L, 0, counts=NULL) == INVALID and b"null pointer" in _err(L)


def test_apply_refusals_and_their_order():
    L = G.lib()
    for P, n_new in ((-1, 10), (1000, -1), (MAX_ROWS, 1), (MAX_ROWS - 5, 6), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _apply(L, P, n_new=n_new) == INVALID and b"bad P/n_new" in _err(L), (P, n_new)
    for M in (0, -1, 17):
        assert _apply(L, M=M) == INVALID and b"bad M" in _err(L), M
    for name in ("kinds", "offsets"):
        assert _apply(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for k, name in enumerate(LEAVES):
        want = b"null tensor pointer (group %d)" % k
        assert _apply(L, **{name: NULL}) == INVALID and want in _err(L), name
        one_null = [None if j == k else ptr().value for j in range(6)]
        assert _apply(L, m=one_null) == INVALID and want in _err(L), name
        assert _apply(L, v=one_null) == INVALID and want in _err(L), name
    for off in (1, 2, 3, 6):
        for name in ("offsets", "stats") + LEAVES:
            assert _apply(L, **{name: ptr(off)}) == INVALID and b"misaligned" in _err(L), (name, off)
        bad = [ptr().value] * 3 + [ptr(off).value] + [ptr().value] * 2
        assert _apply(L, m=bad) == INVALID and b"misaligned" in _err(L)
        assert _apply(L, v=bad) == INVALID and b"misaligned" in _err(L)
    # the order: shape, then null pointers, then alignment
    assert _apply(L, -1, M=0, kinds=NULL) == INVALID and b"bad P/n_new" in _err(L)
    assert _apply(L, M=17, kinds=NULL) == INVALID and b"bad M" in _err(L)
    assert _apply(L, kinds=NULL, xyz=ptr(2)) == INVALID and b"null pointer" in _err(L)
    assert _apply(L, scaling=NULL, xyz=ptr(2)) == INVALID and b"null tensor pointer (group 3)" in _err(L)
    # _features_rest and its moments are not looked at when M == 1, the moment arrays and stats may be null, kinds needs
    # no alignment: each call gets past the null checks and is refused for the one misaligned pointer only
    rest_null = [ptr().value] * 2 + [None] + [ptr().value] * 3
    assert _apply(L, M=1, frest=NULL, m=rest_null, v=rest_null, xyz=ptr(2)) == INVALID and b"misaligned" in _err(L)
    assert _apply(L, M=1, frest=ptr(3), m=None, v=None, stats=NULL, kinds=ptr(1), xyz=ptr(2)) == INVALID
    assert b"misaligned" in _err(L)
    assert _apply(L, M=2, frest=NULL, xyz=ptr(2)) == INVALID and b"null tensor pointer (group 2)" in _err(L)
    # nothing to do is no error and touches nothing (no pointer is looked at)
    nothing = {n: NULL for n in ("kinds", "offsets", "stats") + LEAVES}
    assert _apply(L, 0, n_new=0, m=None, v=None, **nothing) == 0
    assert _apply(L, 0, n_new=5, m=None, v=None, **nothing) == 0
    assert _apply(L, 1000, n_new=0, m=None, v=None, **nothing) == 0
