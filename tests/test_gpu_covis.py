"""GPU tests of keyframe covisibility (csrc/covis.hip through gsr_visibility_pack / gsr_covisibility /
gsr_observation_count / gsr_visibility_remap, gs_livm_amd.KeyframeVisibility, GrowableGaussians.attach_visibility).
Everything is integer arithmetic: every comparison is torch.equal against tests/covis_ref.py."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import covis_ref as V
from arena import Arena, offsets

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def _i64(a):
    """uint64 numpy words as the int64 tensor the library's hosts take"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def _guarded_words(A, name, n):
    """n int64 words inside a guarded allocation of their own (tests/arena.py), pre-filled with 0xFF.. : every word the
    call is to write is written, and nothing either side of them"""
    t = A.put(name, shape=(2 * n,)).view(torch.int64)
    t.fill_(-1)
    return t


def _guarded_i32(A, name, n):
    t = A.put(name, shape=(n,)).view(torch.int32)
    t.fill_(0x5A5A5A5A)
    return t


def _slab_with_gap(rows, dev, gap=5):
    """the rows as a [n, words] view of a [n, words + gap] slab: a pitch larger than `words`, the gap all ones"""
    n, words = rows.shape
    slab = torch.full((n, words + gap), -1, dtype=torch.int64, device=dev)
    slab[:, :words] = _i64(rows).to(dev)
    return slab[:, :words]


# ---- pack -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", V.PACK_SIZES)
def test_pack_writes_every_word_and_clears_the_tail(P, gpu_device):
    dev = gpu_device
    sources = [V.radii_case(P), V.mask_case(P), V.mask_case(P, 1, dtype=bool)]
    assert sources[0].dtype == np.int32 and sources[1].dtype == np.uint8 and sources[2].dtype == bool
    if P >= 255:     # negative radii, zeros, INT_MAX and INT_MIN all occur; so do mask bytes other than 0 and 1
        assert {0, V.INT_MAX, -V.INT_MAX - 1} <= set(sources[0].tolist()) and (sources[0] < 0).any()
        assert {0, 1, 0x80, 0xFF} <= set(sources[1].tolist())
    for k, src in enumerate(sources):
        seen = V.seen_from(src)
        for extra in (0, 3):
            words = V.words_of(P) + extra
            A = Arena(dev, offsets("a8" if (k + extra) % 2 else "a0"))
            row = _guarded_words(A, "row", words)
            out = G.visibility_pack(torch.from_numpy(src).to(dev), out=row, words=words)
            want = _i64(V.pack_ref(seen, words)).to(dev)
            assert out.data_ptr() == row.data_ptr() and torch.equal(row, want), (P, k, extra)
            assert A.guards_intact() is None
    # a new row of the default length; INT_MAX is seen, INT_MIN and 0 are not
    r = torch.tensor([V.INT_MAX, -V.INT_MAX - 1, 0, 1, -1], dtype=torch.int32, device=dev)
    assert G.visibility_pack(r).tolist() == [0b01001]


# ---- overlap ------------------------------------------------------------------------------------------------------------
KINDS = ("zeros", "ones", "0.01", "0.5")


def _mixed_rows(n, words, seed, tail_bits):
    """row r is of kind KINDS[r % 4]; the last word's top tail_bits bits are clear (P = 64 words - tail_bits)"""
    return np.concatenate([V.rows_case(1, words, KINDS[(r + seed) % 4], seed=100 * seed + r, tail_bits=tail_bits)
                           for r in range(n)])


@pytest.mark.parametrize("words", [1, 4, 17, 3126])
@pytest.mark.parametrize("Q,K,same", [(1, 1, False), (1, 50, False), (7, 9, False), (9, 9, True), (65, 3, False)])
def test_overlap_counts_are_exact(Q, K, same, words, gpu_device):
    dev, tail = gpu_device, 13
    P = 64 * words - tail
    q_np = _mixed_rows(Q, words, 1, tail)
    k_np = q_np if same else _mixed_rows(K, words, 2, tail)
    inter, qc, kc = V.overlap_ref(q_np, k_np)
    assert P in qc.tolist() or Q < 2                                  # an all-ones row counts P
    if Q >= 4 and K >= 4:
        assert 0 in qc.tolist() and P in kc.tolist() and (inter > 0).any()
    q = _slab_with_gap(q_np, dev)
    k = None if same else _slab_with_gap(k_np, dev, gap=2)
    assert q.stride(0) == words + 5
    want = [torch.from_numpy(x).to(dev) for x in (inter, qc, kc)]
    A = Arena(dev, offsets("mix"))
    out = (_guarded_i32(A, "inter", Q * K), _guarded_i32(A, "qc", Q), _guarded_i32(A, "kc", K))   # garbage inside
    got = G.covisibility(q, k, words=words, out=out)
    assert torch.equal(got[0].view(Q, K), want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert A.guards_intact() is None
    again = G.covisibility(q, k, words=words)                          # new tensors; and the same counts once more
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(again, got))
    if same:
        assert torch.equal(torch.diagonal(again[0]), again[1]) and torch.equal(again[1], again[2])
    # without the count outputs: only inter is written
    B = Arena(dev, offsets("a4"))
    only = _guarded_i32(B, "inter", Q * K)
    res = G.covisibility(q, k, words=words, counts=False, out=(only, None, None))
    assert res[1] is None and res[2] is None and torch.equal(only.view(Q, K), want[0]) and B.guards_intact() is None


def test_overlap_of_one_row_tensors_and_fewer_words(gpu_device):
    dev = gpu_device
    rows = V.rows_case(3, 6, "0.5", seed=4)
    t = _i64(rows).to(dev)
    inter, qc, kc = G.covisibility(t[1], t)                           # a 1-D tensor is one query row
    want = V.overlap_ref(rows[1:2], rows)
    assert inter.tolist() == want[0].tolist() and qc.tolist() == want[1].tolist() and kc.tolist() == want[2].tolist()
    inter, qc, kc = G.covisibility(t, words=2)                        # only the first two words of each row count
    want = V.overlap_ref(rows[:, :2], rows[:, :2])
    assert inter.tolist() == want[0].tolist() and qc.tolist() == want[1].tolist()


# ---- count and drop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 50, 65])
def test_observation_count_and_drop(K, gpu_device):
    dev = gpu_device
    for P in V.PACK_SIZES:
        rows = V.visibility_case(K, P)
        count_np = V.count_ref(rows, P)
        assert P < 255 or (0 in count_np.tolist() and K in count_np.tolist())
        bits = _slab_with_gap(rows, dev, gap=3)
        want_count = torch.from_numpy(count_np).to(dev)
        A = Arena(dev, offsets("a4"))
        count = _guarded_i32(A, "count", P)
        got = G.observation_count(bits, P, out=(count, None))          # the count alone
        assert got[1] is None and torch.equal(count, want_count) and A.guards_intact() is None
        for first_row in (0, 64, P - 1, P):
            for min_count in (0, 1, 3, K + 1):
                want_drop = torch.from_numpy(V.drop_ref(count_np, first_row, min_count)).to(dev)
                guard = torch.full((P + 32,), 0xA5, dtype=torch.uint8, device=dev)
                drop = guard[16:16 + P]
                got = G.observation_count(bits, P, first_row, min_count, out=(None, drop))   # the mask alone
                assert got[0] is None and torch.equal(drop, want_drop), (P, first_row, min_count)
                assert bool((guard[:16] == 0xA5).all()) and bool((guard[16 + P:] == 0xA5).all())
                c2, d2 = G.observation_count(bits, P, first_row, min_count, want_count=True, want_drop=True)
                assert torch.equal(c2, want_count) and torch.equal(d2, want_drop)
                if min_count == K + 1:                                  # nobody is seen by K + 1 keyframes
                    assert int(want_drop.sum()) == max(P - first_row, 0)
                if min_count == 0:
                    assert not want_drop.any()


# ---- remap ----------------------------------------------------------------------------------------------------------------
def _marks(P, drop_np, dev):
    """reasons and row_map of the real prune_mark for leaves that all survive the rule, and a caller mask"""
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    rot = z(P, 4)
    rot[:, 0] = 1.0
    reasons, row_map, counts = _capi.prune_mark(z(P, 3), z(P, 3) - 3.0, rot, z(P, 1), drop=torch.from_numpy(drop_np).to(dev))
    assert torch.equal(reasons != 0, torch.from_numpy(drop_np != 0).to(dev))
    return reasons, row_map, int(counts[0])


def _check_remap(P, pattern, dev, K=3):
    drop_np = V.drop_case(P, pattern)
    keep = drop_np == 0
    reasons, row_map, P_new = _marks(P, drop_np, dev)
    assert P_new == int(keep.sum())
    rows = V.visibility_case(K, P, seed=5)
    src = _slab_with_gap(rows, dev, gap=2)
    for dst_words, gap in ((max(V.words_of(P_new), 1), 0), (V.words_of(P) + 2, 3)):
        A = Arena(dev, offsets("a8" if gap else "a0"))
        slab = _guarded_words(A, "dst", K * (dst_words + gap)).view(K, dst_words + gap)
        dst = slab[:, :dst_words]
        out = G.visibility_remap(src, reasons, row_map, dst=dst, dst_words=dst_words)
        want = _i64(V.remap_ref(rows, keep, dst_words)).to(dev)
        assert out.data_ptr() == dst.data_ptr() and torch.equal(dst, want), (P, pattern, dst_words)
        assert bool((slab[:, dst_words:] == -1).all()) and A.guards_intact() is None     # the pitch gap is not written
        assert V.unpack_ref(want.cpu().numpy().view(np.uint64))[:, P_new:].sum() == 0      # nothing beyond P'
    assert torch.equal(src, _i64(rows).to(dev))                                            # out of place
    return P_new


@pytest.mark.parametrize("pattern", V.DROP_PATTERNS)
def test_remap_follows_the_compaction(pattern, gpu_device):
    sizes = V.remap_sizes(pattern)
    landed = [_check_remap(P, pattern, gpu_device) for P in sizes]
    if pattern == "all":
        assert landed == [0, 0, 0]
    else:
        b = landed[1]
        assert b % 64 == 0 and landed == [b - 1, b, b + 1]     # one before, on and one after a word boundary


def test_remap_across_many_workgroups(gpu_device):
    P_new = _check_remap(200_003, "0.3", gpu_device, K=2)
    assert 0.6 * 200_003 < P_new < 0.8 * 200_003
    # a new destination of the default length
    dev, P = gpu_device, 1025
    drop_np = V.drop_case(P, "0.3")
    reasons, row_map, _ = _marks(P, drop_np, dev)
    rows = V.visibility_case(4, P)
    out = G.visibility_remap(_i64(rows).to(dev), reasons, row_map)
    assert tuple(out.shape) == (4, V.words_of(P)) and torch.equal(out, _i64(V.remap_ref(rows, drop_np == 0, V.words_of(P))).to(dev))


# ---- the class ------------------------------------------------------------------------------------------------------------
def test_keyframe_visibility_grows_removes_and_queries(gpu_device):
    dev = gpu_device
    vis = G.KeyframeVisibility(100, keyframes=2, device=dev)
    assert len(vis) == 0 and vis.rows == 100 and vis.words == 2
    with pytest.raises(ValueError):
        vis.overlap()
    srcs = [V.radii_case(100, 1), V.mask_case(100, 2), V.mask_case(100, 3, dtype=bool)]
    for k, s in enumerate(srcs):                                       # the third record doubles the keyframe capacity
        assert vis.record(torch.from_numpy(s).to(dev)) == k
    want = [V.pack_ref(V.seen_from(s)) for s in srcs]
    assert len(vis) == 3 and torch.equal(vis.bits, _i64(np.stack(want)).to(dev))
    # the model grows: a longer record widens the slab, old rows keep their bits and read 0 for the new model rows
    long = V.radii_case(1000, 4)
    assert vis.record(torch.from_numpy(long).to(dev)) == 3 and vis.rows == 1000 and vis.words == 16
    want = [V.pack_ref(V.seen_from(s), 16) for s in srcs] + [V.pack_ref(V.seen_from(long))]
    assert torch.equal(vis.bits, _i64(np.stack(want)).to(dev))
    assert not vis.bits[:3, 2:].any()
    # overwrite slot 1 with a SHORTER source (the model shrank and was rendered again): no stale bit stays
    short = V.radii_case(70, 5)
    assert vis.record(torch.from_numpy(short).to(dev), slot=1) == 1 and len(vis) == 4 and vis.rows == 1000
    want[1] = V.pack_ref(V.seen_from(short), 16)
    assert torch.equal(vis.bits, _i64(np.stack(want)).to(dev))
    # queries: all against all, one slot, a tensor that is packed and not recorded
    ref = V.overlap_ref(np.stack(want), np.stack(want))
    got = vis.overlap()
    assert all(torch.equal(g.cpu(), torch.from_numpy(r)) for g, r in zip(got, ref))
    one = vis.overlap(2)
    assert torch.equal(one[0].cpu(), torch.from_numpy(ref[0][2:3])) and int(one[1]) == int(ref[1][2])
    probe = V.mask_case(1000, 6)
    by_tensor = vis.overlap(torch.from_numpy(probe).to(dev))
    assert len(vis) == 4
    slot = vis.record(torch.from_numpy(probe).to(dev))
    by_slot = vis.overlap(slot)
    assert torch.equal(by_tensor[0], by_slot[0][:, :4]) and torch.equal(by_tensor[1], by_slot[1])
    assert torch.equal(by_tensor[2], by_slot[2][:4]) and int(by_slot[0][0, 4]) == int(by_slot[1])
    want.append(V.pack_ref(V.seen_from(probe)))
    count_np = V.count_ref(np.stack(want), 1000)
    assert torch.equal(vis.observation_count().cpu(), torch.from_numpy(count_np))
    assert torch.equal(vis.unobserved(2, first_row=100).cpu(), torch.from_numpy(V.drop_ref(count_np, 100, 2)))
    # rows the records do not reach yet (the model grew, nobody has rendered it): count 0
    c = vis.observation_count(P=1100)
    assert tuple(c.shape) == (1100,) and torch.equal(c[:1000].cpu(), torch.from_numpy(count_np)) and not c[1000:].any()
    # remove: the last row moves into the hole
    vis.remove(1)
    want[1] = want.pop()
    assert len(vis) == 4 and torch.equal(vis.bits[:, :16], _i64(np.stack(want)).to(dev))
    vis.remove(3)
    assert len(vis) == 3 and torch.equal(vis.bits[:, :16], _i64(np.stack(want[:3])).to(dev))
    with pytest.raises(IndexError):
        vis.remove(3)


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model(sc, dev):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    op = tt(sc["opacities"]).double()
    L = {"_xyz": tt(sc["means3D"]), "_features_dc": tt(sc["shs"][:, :1]), "_features_rest": tt(sc["shs"][:, 1:]),
         "_scaling": torch.log(tt(sc["scales"])), "_rotation": tt(sc["rotations"]) * 1.7,
         "_opacity": torch.log(op / (1 - op)).float()}
    P = L["_xyz"].shape[0]
    m = G.GrowableGaussians(P + 64, 1, dev)
    for n in NAMES:
        m._buf[n][:P].copy_(L[n])
    m.P = P
    m._bind()
    return m


def test_model_prunes_what_no_keyframe_sees_and_the_records_follow(gpu_device):
    dev = gpu_device
    scenes = V.model_scenes()
    P, K, W, H = V.MODEL_P, len(scenes), V.MODEL_W, V.MODEL_H
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    m, twin = _model(scenes[0], dev), _model(scenes[0], dev)
    settings = [G.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], tt(sc["bg"]), 1.0, tt(sc["viewmatrix"]),
                                                tt(sc["projmatrix"]), 0, tt(sc["campos"]), False, False) for sc in scenes]

    def render(model, s):
        with torch.no_grad():
            xyz, opac, scales, rot, shs = model.activated()
            color, radii, depth, acc = G.GaussianRasterizer(s)(xyz, torch.zeros_like(xyz), opac, shs=shs, scales=scales,
                                                                rotations=rot)
        return color, depth, acc, radii

    vis = G.KeyframeVisibility(P, keyframes=4, device=dev)
    m.attach_visibility(vis)
    # one-chain frames, like the other modules' helper frames: these small renders must not feed the calling thread's
    # near/far history, which later tests' large frames start from
    prev = G.set_near_far_thread(False)
    try:
        before = [render(m, s) for s in settings]
        for f in before:
            vis.record(f[3])
        radii = np.stack([f[3].cpu().numpy() for f in before])
        rows = np.stack([V.pack_ref(V.seen_from(r)) for r in radii])
        inter, qc, kc = V.overlap_ref(rows, rows)
        got = vis.overlap()
        assert all(torch.equal(g.cpu(), torch.from_numpy(r)) for g, r in zip(got, (inter, qc, kc)))
        # not vacuous (test_covis_ref.py holds the same on the CPU oracle's radii)
        assert any(0 < inter[a, b] < min(qc[a], qc[b]) for a in range(K) for b in range(K) if a != b)
        count_np = V.count_ref(rows, P)
        assert (count_np == 0).sum() >= 0.05 * P and (count_np == K).sum() >= 0.05 * P
        drop = vis.unobserved(1)
        assert torch.equal(drop.cpu(), torch.from_numpy(V.drop_ref(count_np, 0, 1)))
        out = m.prune(drop=drop)
        keep = (out["reasons"] == 0).cpu().numpy()
        assert np.array_equal(keep, count_np > 0) and m.P == out["P_after"] == int(keep.sum()) < P
        assert vis.rows == m.P and len(vis) == K
        assert torch.equal(vis.bits, _i64(V.remap_ref(rows, keep, V.words_of(m.P))).to(dev))
        after = [render(m, s) for s in settings]
        for b, a in zip(before, after):
            assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[1]) and torch.equal(b[2], a[2])
            assert torch.equal(a[3], b[3][torch.from_numpy(keep).to(dev)])
        repacked = torch.stack([G.visibility_pack(a[3]) for a in after])
        assert torch.equal(repacked, vis.bits)
        assert int(vis.observation_count().min()) >= 1
    finally:
        G.set_near_far_thread(prev)
    # a model without an attachment prunes to the identical leaves
    out2 = twin.prune(drop=drop)
    assert twin.P == m.P and torch.equal(out2["reasons"], out["reasons"]) and torch.equal(out2["row_map"], out["row_map"])
    for n in NAMES:
        assert torch.equal(getattr(twin, n), getattr(m, n)), n
    # a prune that drops nothing leaves the records alone
    slab = vis._slab
    again = m.prune(drop=vis.unobserved(1))
    assert again["P_after"] == again["P_before"] and vis._slab is slab
