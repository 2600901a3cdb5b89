"""GPU tests of the C++/LibTorch route of keyframe covisibility (csrc/torch_next.cpp: visibility_pack, covisibility,
observation_count, visibility_remap) against the Python route (gs-livm_amd/covis.py over _capi).  Both launch the same
kernels with the same arguments: results must be bit-identical, and both equal tests/covis_ref.py."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import covis_ref as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx(gpu_device):
    return G.torch_ops().next


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_pack_matches_the_python_route(nx, gpu_device):
    dev, P = gpu_device, 1025
    for src in (V.radii_case(P), V.mask_case(P), V.mask_case(P, 1, dtype=bool)):
        t = torch.from_numpy(src).to(dev)
        for words in (0, V.words_of(P) + 3):
            x = nx.visibility_pack(t, words)
            y = G.visibility_pack(t, words=words or None)
            assert _same(x, y) and torch.equal(x, _i64(V.pack_ref(V.seen_from(src), words or None)).to(dev))


def test_covisibility_matches_the_python_route(nx, gpu_device):
    dev, words = gpu_device, 17
    q_np, k_np = V.rows_case(7, words, "0.5", seed=1, tail_bits=13), V.rows_case(9, words, "0.5", seed=2, tail_bits=13)
    slab = torch.full((9, words + 4), -1, dtype=torch.int64, device=dev)       # a pitch larger than the rows
    slab[:, :words] = _i64(k_np).to(dev)
    q, k = _i64(q_np).to(dev), slab[:, :words]
    want = [torch.from_numpy(x).to(dev) for x in V.overlap_ref(q_np, k_np)]
    x, y = nx.covisibility(q, k), G.covisibility(q, k)
    assert all(_same(a, b) and torch.equal(a, w) for a, b, w in zip(x, y, want))
    x, y = nx.covisibility(k, None, 0, False), G.covisibility(k, counts=False)  # the keyframes against themselves
    assert _same(x[0], y[0]) and x[1] is None and x[2] is None and y[1] is None
    assert torch.equal(x[0], torch.from_numpy(V.overlap_ref(k_np, k_np)[0]).to(dev))


def test_observation_count_matches_the_python_route(nx, gpu_device):
    dev, K, P = gpu_device, 50, 1025
    rows = V.visibility_case(K, P)
    bits = _i64(rows).to(dev)
    count_np = V.count_ref(rows, P)
    for first_row, min_count in ((0, 1), (64, 3), (P, K + 1)):
        x = nx.observation_count(bits, P, first_row, min_count, True, True)
        y = G.observation_count(bits, P, first_row, min_count, want_count=True, want_drop=True)
        assert _same(x[0], y[0]) and _same(x[1], y[1])
        assert torch.equal(x[0].cpu(), torch.from_numpy(count_np))
        assert torch.equal(x[1].cpu(), torch.from_numpy(V.drop_ref(count_np, first_row, min_count)))
    x = nx.observation_count(bits, P, 0, 2, False, True)
    assert x[0] is None and torch.equal(x[1].cpu(), torch.from_numpy(V.drop_ref(count_np, 0, 2)))
    with pytest.raises(Exception):
        nx.observation_count(bits, P, 0, 2, False, False)            # neither output: refused by the library


def test_remap_matches_the_python_route(nx, gpu_device):
    dev, K, P = gpu_device, 3, 1025
    drop_np = V.drop_case(P, "0.3")
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    rot = z(P, 4)
    rot[:, 0] = 1.0
    drop = torch.from_numpy(drop_np).to(dev)
    reasons, row_map, counts = nx.prune_mark(z(P, 3), z(P, 3) - 3.0, rot, z(P, 1), drop=drop)
    r2, m2, _ = _capi.prune_mark(z(P, 3), z(P, 3) - 3.0, rot, z(P, 1), drop=drop)
    assert _same(reasons, r2) and _same(row_map, m2) and int(counts[0]) == int((drop_np == 0).sum())
    rows = V.visibility_case(K, P, seed=5)
    src = _i64(rows).to(dev)
    for dst_words in (0, V.words_of(int(counts[0])), V.words_of(P) + 2):
        x = nx.visibility_remap(src, reasons, row_map, dst_words)
        y = G.visibility_remap(src, reasons, row_map, dst_words=dst_words or None)
        want = _i64(V.remap_ref(rows, drop_np == 0, dst_words or V.words_of(P))).to(dev)
        assert _same(x, y) and torch.equal(x, want)
