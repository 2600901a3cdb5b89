"""Reference for csrc/covis.hip (keyframe covisibility) in numpy, and the inputs the GPU and C++ tests share.

The packed form is np.packbits(..., bitorder="little") viewed as uint64: bit i % 64 of word i // 64 is model row i.  An
independent slow form keeps a row as a Python set of row numbers; test_covis_ref.py holds the two against each other.
Everything is integer arithmetic, so every comparison in the tests is an equality.  numpy only; every generator is
deterministic in its arguments."""
import numpy as np

INT_MAX = 2 ** 31 - 1
# every seam of the 64-row words and of the four words a workgroup counts or remaps; 1 025 rows are a wave's eight words
# of k_visibility_pack twice over and one more; 200 003 rows are many workgroups of every kernel and a partial last one
PACK_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 200_003)
MODEL_P, MODEL_W, MODEL_H, MODEL_SEED = 3000, 64, 48, 21
# 36 degree views of a scene laid out for 60: they share a core, each sees a strip of its own, and about half of the rows
# lie outside all of them
MODEL_FOVX, MODEL_YAWS = 36.0, (-10.0, -5.0, 0.0, 5.0, 10.0)


def words_of(P):
    return (int(P) + 63) // 64


# ---- the packed form ----------------------------------------------------------------------------------------------------
def seen_from(src):
    """the visibility a source means: radii > 0 for an integer array, != 0 for a mask"""
    src = np.asarray(src).reshape(-1)
    return src > 0 if src.dtype == np.int32 else src != 0


def pack_ref(seen, words=None):
    """[words] uint64 of a bool [P]; words beyond ceil(P / 64) and the bits at and beyond P are zero"""
    seen = np.asarray(seen, dtype=bool).reshape(-1)
    words = words_of(seen.size) if words is None else int(words)
    assert words >= words_of(seen.size)
    full = np.zeros(words * 64, dtype=bool)
    full[:seen.size] = seen
    return np.packbits(full, bitorder="little").view(np.uint64).copy()


def unpack_ref(bits, P=None):
    """bool [..., P] of uint64 [..., words]"""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little").astype(bool)
    return out if P is None else out[..., :P]


def overlap_ref(q_bits, k_bits):
    """(inter [Q,K], q_count [Q], k_count [K]) int32 of uint64 [Q,words] and [K,words]"""
    q, k = unpack_ref(q_bits), unpack_ref(k_bits)
    inter = np.array([[np.count_nonzero(a & b) for b in k] for a in q], dtype=np.int32).reshape(len(q), len(k))
    return inter, q.sum(1).astype(np.int32), k.sum(1).astype(np.int32)


def count_ref(bits, P):
    """[P] int32: how many of the K rows have bit i set"""
    return unpack_ref(bits, P).sum(0).astype(np.int32)


def drop_ref(count, first_row, min_count):
    i = np.arange(count.size)
    return ((i >= first_row) & (count < min_count)).astype(np.uint8)


def remap_ref(bits, keep, dst_words):
    """the compaction of every row: [K, dst_words] uint64 of uint64 [K, >= ceil(P / 64)] and keep bool [P]"""
    keep = np.asarray(keep, dtype=bool)
    rows = unpack_ref(bits, keep.size)
    return np.stack([pack_ref(r[keep], dst_words) for r in rows]) if len(rows) else np.zeros((0, dst_words), np.uint64)


# ---- the slow form: a row as a set of row numbers -------------------------------------------------------------------
def set_of(seen):
    return {i for i, s in enumerate(np.asarray(seen).reshape(-1)) if s}


def set_of_words(bits):
    return {64 * w + b for w, word in enumerate(bits) for b in range(64) if (int(word) >> b) & 1}


def overlap_sets(q_sets, k_sets):
    inter = [[len(a & b) for b in k_sets] for a in q_sets]
    return inter, [len(a) for a in q_sets], [len(b) for b in k_sets]


def count_sets(sets, P):
    return [sum(i in s for s in sets) for i in range(P)]


def remap_set(s, keep):
    new_row, out = 0, set()
    for i, k in enumerate(keep):
        if k:
            if i in s:
                out.add(new_row)
            new_row += 1
    return out


# ---- ratios (what gs_livm_amd.iou / overlap_coefficient compute), in plain Python ------------------------------------
def iou_ref(inter, qc, kc):
    return [[(i / (a + b - i) if a + b - i else 0.0) for i, b in zip(row, kc)] for row, a in zip(inter, qc)]


def overlap_coefficient_ref(inter, qc, kc):
    return [[(i / min(a, b) if min(a, b) else 0.0) for i, b in zip(row, kc)] for row, a in zip(inter, qc)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def radii_case(P, seed=0):
    """int32 [P]: zeros, positive and negative radii, INT_MAX and INT_MIN among them, in no pattern a word repeats"""
    rng = np.random.default_rng(7919 * P + seed)
    r = rng.integers(1, 400, P).astype(np.int32)
    kind = rng.integers(0, 6, P)
    r[kind == 0] = 0
    r[kind == 1] = -r[kind == 1]
    r[kind == 2] = INT_MAX
    r[kind == 3] = -INT_MAX - 1
    return r


def mask_case(P, seed=0, dtype=np.uint8):
    """[P] uint8 with 0, 1 and other non-zero bytes (0x80, 0xFF), or bool"""
    rng = np.random.default_rng(104729 * P + seed)
    m = rng.choice(np.array([0, 0, 1, 2, 0x80, 0xFF], dtype=np.uint8), P)
    return m != 0 if dtype == bool else m


def rows_case(n, words, kind, seed=0, tail_bits=0):
    """uint64 [n, words]: "zeros", "ones", or random at a density ("0.01", "0.5").  tail_bits: that many of the last
    word's top bits are cleared (rows of a model whose P is no multiple of 64)."""
    total = words * 64 - tail_bits
    if kind == "zeros":
        seen = np.zeros((n, total), dtype=bool)
    elif kind == "ones":
        seen = np.ones((n, total), dtype=bool)
    else:
        rng = np.random.default_rng(31 * n + 1009 * words + seed)
        seen = rng.random((n, total)) < float(kind)
    return np.stack([pack_ref(s, words) for s in seen])


def visibility_case(K, P, seed=0):
    """uint64 [K, ceil(P / 64)]: K keyframes' rows over P model rows at mixed densities; a tenth of the rows is seen by
    nobody and a tenth by everybody, so counts 0 and K occur"""
    rng = np.random.default_rng(613 * K + 17 * P + seed)
    dens = rng.uniform(0.05, 0.9, (K, 1))
    seen = rng.random((K, P)) < dens
    cls = rng.integers(0, 10, P)
    seen[:, cls == 0] = False
    seen[:, cls == 1] = True
    return np.stack([pack_ref(s) for s in seen])


DROP_PATTERNS = ("none", "all", "alternating", "first64", "last", "0.3")


def drop_case(P, pattern, seed=0):
    """the caller's prune mask, uint8 [P]"""
    d = np.zeros(P, dtype=np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "alternating":
        d[::2] = 1
    elif pattern == "first64":
        d[:64] = 1
    elif pattern == "last":
        d[-1] = 1
    elif pattern != "none":
        d[np.random.default_rng(P + seed).random(P) < float(pattern)] = 1
    return d


def remap_sizes(pattern):
    """three model sizes P at which the pattern leaves P' one before, on and one after a word boundary"""
    if pattern in ("none", "all"):
        return (127, 128, 129)          # ("all": P' = 0 whatever P; the sizes straddle the source's word boundary)
    if pattern == "alternating":
        return (254, 256, 258)          # the even rows leave: P' = P / 2
    if pattern == "first64":
        return (191, 192, 193)
    if pattern == "last":
        return (128, 129, 130)
    out = []
    for target in (255, 256, 257):      # a random pattern: the first size from 300 on that hits the target
        out.append(next(P for P in range(300, 800) if int((drop_case(P, pattern) == 0).sum()) == target))
    return tuple(out)


def model_scenes():
    """the synthetic scene of the model-level test seen from MODEL_YAWS: a list of scene dicts that share the Gaussians"""
    from gs_livm_amd import synthetic as S
    base = S.make_scene(MODEL_P, MODEL_W, MODEL_H, MODEL_SEED, sh_degree=0)
    out = []
    for yaw in MODEL_YAWS:
        sc = dict(base)
        sc.update(S.make_camera(MODEL_W, MODEL_H, fovx_deg=MODEL_FOVX, yaw_deg=yaw))
        out.append(sc)
    return out
