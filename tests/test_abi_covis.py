"""CPU tests of the argument validation of the covisibility entry points (gsr_visibility_words, gsr_visibility_pack,
gsr_covisibility, gsr_observation_count, gsr_visibility_remap): no device involved -- validation comes first, and nothing
is enqueued or written on a refusal -- and of what the feature registers (symbols, the one profiler id, Python names)."""
import ctypes as C

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1                  # GSR_ERR_INVALID_ARGUMENT
MAX_WORDS = (2 ** 31 - 1) // 64   # words * 64 stays an int32


def ptr(offset=0, base=1 << 20):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(base + offset)


def _err(L):
    return L.gsr_last_error()


def _pack(L, P=1000, words=None, radii=ptr(), mask=NULL, bits=ptr(0, 2 << 20)):
    words = (P + 63) // 64 if words is None else words
    return L.gsr_visibility_pack(P, radii, mask, bits, words, NULL)


def _overlap(L, Q=3, K=5, words=16, q_bits=ptr(), k_bits=ptr(0, 2 << 20), q_pitch=None, k_pitch=None,
             inter=ptr(0, 3 << 20), q_count=ptr(0, 4 << 20), k_count=ptr(0, 5 << 20)):
    return L.gsr_covisibility(Q, q_bits, words if q_pitch is None else q_pitch, K, k_bits,
                              words if k_pitch is None else k_pitch, words, inter, q_count, k_count, NULL)


def _count(L, K=5, P=1000, pitch=None, first_row=0, min_count=1, bits=ptr(), count=ptr(0, 2 << 20),
           drop=ptr(0, 3 << 20)):
    return L.gsr_observation_count(K, bits, (P + 63) // 64 if pitch is None else pitch, P, first_row, min_count, count,
                                   drop, NULL)


def _remap(L, K=5, P=1000, src=ptr(), src_pitch=None, reasons=ptr(0, 3 << 20), row_map=ptr(0, 4 << 20),
           dst=ptr(0, 2 << 20), dst_pitch=None, dst_words=None):
    need = (P + 63) // 64
    dst_words = need if dst_words is None else dst_words
    return L.gsr_visibility_remap(K, src, need if src_pitch is None else src_pitch, P, reasons, row_map, dst,
                                  dst_words if dst_pitch is None else dst_pitch, dst_words, NULL)


def test_symbols_kernel_id_and_python_names_are_registered():
    L = G.lib()
    for n in ("gsr_visibility_words", "gsr_visibility_pack", "gsr_covisibility", "gsr_observation_count",
              "gsr_visibility_remap"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    # ONE id for the four kernels, directly behind k_delta_convert; the profiler mask is one 64-bit word and now full
    assert names.count("k_visibility") == 1 and [k for k in names if k.startswith("k_visibility")] == ["k_visibility"]
    assert names.index("k_visibility") == names.index("k_delta_convert") + 1
    assert len(set(names)) == len(names) == 64 and "" not in names
    assert names.index("k_preprocess") == 0 and names.index("k_model_step") == 27
    assert names[-4:] == ["k_prune_mark", "k_prune_scan", "k_prune_rank", "k_prune_compact"]
    assert L.gsr_kernel_name(64) == b"" and L.gsr_abi_version() == 2
    for n in ("KeyframeVisibility", "visibility_pack", "covisibility", "observation_count", "visibility_remap", "iou",
              "overlap_coefficient"):
        assert n in G.__all__ and hasattr(G, n), n
    assert hasattr(G.GrowableGaussians, "attach_visibility")


def test_visibility_words():
    L = G.lib()
    for P, want in ((0, 0), (-1, 0), (-2 ** 31, 0), (1, 1), (64, 1), (65, 2), (2 ** 31 - 1, 2 ** 25)):
        assert L.gsr_visibility_words(P) == want, P


def test_pack_refusals_and_their_order():
    L = G.lib()
    for P in (0, -1, -2 ** 31):
        assert _pack(L, P, words=4) == INVALID and b"bad P" in _err(L), P
    for P in (1, 64, 65, 200_003):
        need = (P + 63) // 64
        assert _pack(L, P, words=need - 1) == INVALID and b"words too small" in _err(L) and str(need).encode() in _err(L)
    assert _pack(L, 1, words=0) == INVALID and _pack(L, 1, words=-3) == INVALID
    assert _pack(L, 1000, words=MAX_WORDS + 1) == INVALID and b"beyond int32" in _err(L)
    assert _pack(L, 2 ** 31 - 1, words=2 ** 25) == INVALID and b"beyond int32" in _err(L)
    assert _pack(L, radii=ptr(), mask=ptr(64)) == INVALID and b"exactly one" in _err(L)
    assert _pack(L, radii=NULL, mask=NULL) == INVALID and b"exactly one" in _err(L)
    assert _pack(L, bits=NULL) == INVALID and b"null pointer" in _err(L)
    for off in (1, 2, 3, 4, 5, 6, 7, 12):
        assert _pack(L, bits=ptr(off, 2 << 20)) == INVALID and b"8-byte" in _err(L), off
    for off in (1, 2, 3):
        assert _pack(L, radii=ptr(off)) == INVALID and b"4-byte" in _err(L), off
    # the order: shape, the choice of the source, null pointers, alignment (bit pointers first)
    assert _pack(L, 0, words=0, radii=NULL, bits=NULL) == INVALID and b"bad P" in _err(L)
    assert _pack(L, 100, words=1, radii=NULL, bits=NULL) == INVALID and b"words too small" in _err(L)
    assert _pack(L, 100, words=MAX_WORDS + 1, radii=NULL, bits=NULL) == INVALID and b"beyond int32" in _err(L)
    assert _pack(L, radii=NULL, bits=NULL) == INVALID and b"exactly one" in _err(L)
    assert _pack(L, radii=ptr(2), bits=NULL) == INVALID and b"null pointer" in _err(L)
    assert _pack(L, radii=ptr(2), bits=ptr(4, 2 << 20)) == INVALID and b"8-byte" in _err(L)


def test_covisibility_refusals_and_their_order():
    L = G.lib()
    for bad in (0, -1):
        assert _overlap(L, Q=bad) == INVALID and b"bad Q" in _err(L)
        assert _overlap(L, K=bad) == INVALID and b"bad K" in _err(L)
        assert _overlap(L, words=bad, q_pitch=16, k_pitch=16) == INVALID and b"bad words" in _err(L)
    assert _overlap(L, q_pitch=15) == INVALID and b"pitch too small" in _err(L)
    assert _overlap(L, k_pitch=15) == INVALID and b"pitch too small" in _err(L)
    assert _overlap(L, k_pitch=-16) == INVALID and b"pitch too small" in _err(L)
    assert _overlap(L, words=MAX_WORDS + 1) == INVALID and b"words * 64 beyond int32" in _err(L)
    assert _overlap(L, Q=65536, K=32768) == INVALID and b"Q * K beyond int32" in _err(L)
    for name in ("q_bits", "k_bits", "inter"):
        assert _overlap(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for off in (1, 2, 4, 7):
        assert _overlap(L, q_bits=ptr(off)) == INVALID and b"8-byte" in _err(L), off
        assert _overlap(L, k_bits=ptr(off, 2 << 20)) == INVALID and b"8-byte" in _err(L), off
    for name in ("inter", "q_count", "k_count"):
        for off in (1, 2, 3):
            assert _overlap(L, **{name: ptr(off, 6 << 20)}) == INVALID and b"4-byte" in _err(L), (name, off)
    # the order: shape (Q, K, words, pitches, the int32 limits), null pointers, alignment (bit pointers first)
    assert _overlap(L, Q=0, K=0, words=0, q_bits=NULL) == INVALID and b"bad Q" in _err(L)
    assert _overlap(L, K=0, words=0, q_bits=NULL) == INVALID and b"bad K" in _err(L)
    assert _overlap(L, words=0, q_bits=NULL) == INVALID and b"bad words" in _err(L)
    assert _overlap(L, q_pitch=1, words=MAX_WORDS + 1, q_bits=NULL) == INVALID and b"pitch too small" in _err(L)
    assert _overlap(L, Q=65536, K=32768, inter=NULL, q_bits=ptr(4)) == INVALID and b"Q * K" in _err(L)
    assert _overlap(L, inter=NULL, q_bits=ptr(4)) == INVALID and b"null pointer" in _err(L)
    assert _overlap(L, q_bits=ptr(4), inter=ptr(2)) == INVALID and b"8-byte" in _err(L)


def test_observation_count_refusals_and_their_order():
    L = G.lib()
    for bad in (0, -1):
        assert _count(L, K=bad) == INVALID and b"bad K" in _err(L)
        assert _count(L, P=bad, pitch=4) == INVALID and b"bad P" in _err(L)
    for P in (1, 64, 65, 200_003):
        assert _count(L, P=P, pitch=(P + 63) // 64 - 1) == INVALID and b"pitch too small" in _err(L), P
    assert _count(L, P=2 ** 31 - 1, pitch=2 ** 25) == INVALID and b"beyond int32" in _err(L)
    assert _count(L, first_row=-1) == INVALID and b"bad first_row" in _err(L)
    assert _count(L, min_count=-1) == INVALID and b"bad min_count" in _err(L)
    assert _count(L, count=NULL, drop=NULL) == INVALID and b"neither count nor drop" in _err(L)
    assert _count(L, bits=NULL) == INVALID and b"null pointer" in _err(L)
    for off in (1, 4, 7):
        assert _count(L, bits=ptr(off)) == INVALID and b"8-byte" in _err(L), off
    for off in (1, 2, 3):
        assert _count(L, count=ptr(off, 2 << 20)) == INVALID and b"4-byte" in _err(L), off
    # the order: shape, the choice of the outputs, null pointers, alignment (bit pointers first)
    assert _count(L, K=0, P=0, pitch=0, count=NULL, drop=NULL, bits=NULL) == INVALID and b"bad K" in _err(L)
    assert _count(L, P=0, pitch=0, count=NULL, drop=NULL, bits=NULL) == INVALID and b"bad P" in _err(L)
    assert _count(L, pitch=1, first_row=-1, count=NULL, drop=NULL) == INVALID and b"pitch too small" in _err(L)
    assert _count(L, first_row=-1, min_count=-1, count=NULL, drop=NULL) == INVALID and b"bad first_row" in _err(L)
    assert _count(L, min_count=-1, count=NULL, drop=NULL) == INVALID and b"bad min_count" in _err(L)
    assert _count(L, count=NULL, drop=NULL, bits=NULL) == INVALID and b"neither" in _err(L)
    assert _count(L, bits=NULL, count=ptr(2)) == INVALID and b"null pointer" in _err(L)
    assert _count(L, bits=ptr(4), count=ptr(2)) == INVALID and b"8-byte" in _err(L)


def test_remap_refusals_and_their_order():
    L = G.lib()
    for bad in (0, -1):
        assert _remap(L, K=bad) == INVALID and b"bad K" in _err(L)
        assert _remap(L, P=bad, src_pitch=4, dst_words=4) == INVALID and b"bad P" in _err(L)
        assert _remap(L, dst_words=bad, dst_pitch=16) == INVALID and b"bad dst_words" in _err(L)
    assert _remap(L, src_pitch=15) == INVALID and b"pitch too small" in _err(L) and b"16" in _err(L)
    assert _remap(L, dst_words=20, dst_pitch=19) == INVALID and b"pitch too small" in _err(L) and b"20" in _err(L)
    assert _remap(L, dst_words=MAX_WORDS + 1) == INVALID and b"beyond int32" in _err(L)
    for name in ("src", "reasons", "row_map", "dst"):
        assert _remap(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for off in (1, 4, 7):
        assert _remap(L, src=ptr(off)) == INVALID and b"8-byte" in _err(L), off
        assert _remap(L, dst=ptr(off, 2 << 20)) == INVALID and b"8-byte" in _err(L), off
    for off in (1, 2, 3):
        assert _remap(L, row_map=ptr(off, 4 << 20)) == INVALID and b"4-byte" in _err(L), off
    # out of place: the slabs (first word of the first row to the last word of the last row) must not overlap
    K, P = 5, 1000
    span = 8 * (4 * 16 + 16)                                           # pitch 16, four rows and the last row's 16 words
    base = 1 << 20
    for dst in (base, base + 8, base + span - 8, base - span + 8):
        assert _remap(L, K, P, src=ptr(0, base), dst=C.c_void_p(dst)) == INVALID and b"overlap" in _err(L), dst
    # slabs that only touch pass the validation; src rows interleaved with dst rows in one allocation do not
    assert _remap(L, K, P, src=ptr(0, base), dst=C.c_void_p(base + 8 * 16), src_pitch=32, dst_pitch=32) == INVALID
    assert b"overlap" in _err(L)
    # the order: shape, null pointers, alignment (bit pointers first), overlap
    assert _remap(L, K=0, P=0, dst_words=0, src=NULL) == INVALID and b"bad K" in _err(L)
    assert _remap(L, P=0, src_pitch=1, dst_words=0, dst_pitch=1, src=NULL) == INVALID and b"bad P" in _err(L)
    assert _remap(L, dst_words=0, dst_pitch=1, src=NULL) == INVALID and b"bad dst_words" in _err(L)
    assert _remap(L, src_pitch=1, src=NULL) == INVALID and b"pitch too small" in _err(L)
    assert _remap(L, src=NULL, dst=ptr(4)) == INVALID and b"null pointer" in _err(L)
    assert _remap(L, src=ptr(0, base), dst=ptr(4, base), row_map=ptr(2)) == INVALID and b"8-byte" in _err(L)
    assert _remap(L, src=ptr(0, base), dst=ptr(0, base), row_map=ptr(2)) == INVALID and b"4-byte" in _err(L)
    assert _remap(L, src=ptr(0, base), dst=ptr(0, base)) == INVALID and b"overlap" in _err(L)
