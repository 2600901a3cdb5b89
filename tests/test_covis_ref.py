"""CPU tests of the covisibility reference itself (tests/covis_ref.py): the packed numpy form against the slow form that
keeps a row as a Python set, the two ratios against hand values, and the scene of the model-level GPU test, which must
not be vacuous."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from oracle import oracle as O

import covis_ref as V


@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_packed_form_equals_the_set_form(P):
    K = 4
    seen = [V.seen_from(V.radii_case(P, k)) for k in range(K - 1)] + [V.seen_from(V.mask_case(P, 9))]
    rows = np.stack([V.pack_ref(s, V.words_of(P) + 1) for s in seen])          # one spare word: it stays zero
    sets = [V.set_of(s) for s in seen]
    assert rows.dtype == np.uint64 and rows.shape == (K, V.words_of(P) + 1) and not rows[:, -1].any()
    for r, s, b in zip(rows, sets, seen):
        assert V.set_of_words(r) == s and all(i < P for i in s)
        assert np.array_equal(V.unpack_ref(r, P), b)
    inter, qc, kc = V.overlap_ref(rows[:3], rows)
    si, sq, sk = V.overlap_sets(sets[:3], sets)
    assert inter.tolist() == si and qc.tolist() == sq and kc.tolist() == sk
    count = V.count_ref(rows, P)
    assert count.tolist() == V.count_sets(sets, P)
    for first_row, min_count in ((0, 1), (P // 2, 2), (P, 3), (0, 0)):
        want = [int(i >= first_row and c < min_count) for i, c in enumerate(count.tolist())]
        assert V.drop_ref(count, first_row, min_count).tolist() == want
    for pattern in V.DROP_PATTERNS:
        keep = V.drop_case(P, pattern) == 0
        out = V.remap_ref(rows, keep, V.words_of(P))
        for r, s in zip(out, sets):
            assert V.set_of_words(r) == V.remap_set(s, keep)


def test_ratios_against_hand_values():
    inter = torch.tensor([[2, 0, 0], [3, 4, 0]], dtype=torch.int32)
    qc = torch.tensor([4, 6], dtype=torch.int32)
    kc = torch.tensor([6, 4, 0], dtype=torch.int32)
    iou = G.iou(inter, qc, kc)
    oc = G.overlap_coefficient(inter, qc, kc)
    assert iou.dtype == oc.dtype == torch.float64 and iou.shape == oc.shape == (2, 3)
    assert iou.tolist() == [[2 / 8, 0.0, 0.0], [3 / 9, 4 / 6, 0.0]]
    assert oc.tolist() == [[2 / 4, 0.0, 0.0], [3 / 6, 4 / 4, 0.0]]
    assert iou.tolist() == V.iou_ref(inter.tolist(), qc.tolist(), kc.tolist())
    assert oc.tolist() == V.overlap_coefficient_ref(inter.tolist(), qc.tolist(), kc.tolist())
    zero = torch.zeros((1, 1), dtype=torch.int32)                        # 0 / 0 = 0, not NaN
    assert G.iou(zero, zero[0], zero[0]).tolist() == [[0.0]]
    assert G.overlap_coefficient(zero, zero[0], zero[0]).tolist() == [[0.0]]
    # a row against itself: both ratios are 1
    assert G.iou(qc[:1].reshape(1, 1), qc[:1], qc[:1]).tolist() == [[1.0]]
    assert G.overlap_coefficient(qc[:1].reshape(1, 1), qc[:1], qc[:1]).tolist() == [[1.0]]


def test_model_scene_is_not_vacuous():
    """The views of the model-level GPU test, rendered by the CPU oracle: some pair overlaps partly, at least 5 % of the
    rows are seen by no keyframe and at least 5 % by every keyframe -- the GPU test cannot pass on an empty overlap."""
    scenes = V.model_scenes()
    K, P = len(scenes), V.MODEL_P
    assert K == 5
    rows = np.stack([V.pack_ref(V.seen_from(O.forward(sc, keep_handle=False).radii.astype(np.int32))) for sc in scenes])
    inter, qc, kc = V.overlap_ref(rows, rows)
    assert np.array_equal(np.diag(inter), qc) and np.array_equal(qc, kc) and (qc > 0).all()
    partial = [(a, b) for a in range(K) for b in range(K)
               if a != b and 0 < inter[a, b] < min(qc[a], qc[b])]
    assert partial, inter
    count = V.count_ref(rows, P)
    assert (count == 0).sum() >= 0.05 * P, (count == 0).sum()
    assert (count == K).sum() >= 0.05 * P, (count == K).sum()
    assert 0 < V.drop_ref(count, 0, 1).sum() < P
