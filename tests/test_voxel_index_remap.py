"""CPU tests of VoxelIndex.remap (gs-livm_amd/model.py): a voxel's row range after a stable compaction of the model's
rows, against brute force -- every range expanded to its row list, filtered by keep, renumbered."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
import prune_ref as R


def _index(seed, nvox=300):
    """random voxels laid out back to back, about a fifth of them empty; returns (index, keys, counts, P)"""
    rng = np.random.RandomState(seed)
    keys = (rng.permutation(100_000)[:nvox].astype(np.int64) * 9973 + 17).tolist()   # distinct
    counts = rng.randint(0, 9, size=nvox)
    counts[rng.rand(nvox) < 0.2] = 0
    counts[0] = 0          # an empty voxel at row 0 ...
    counts[-1] = 0         # ... and one whose first row is P
    vi = G.VoxelIndex()
    P = vi.add(keys, counts.tolist(), 0)
    assert P == int(counts.sum())
    return vi, keys, counts.tolist(), P


def _keeps(P, seed):
    rng = np.random.RandomState(seed)
    alt = (np.arange(P) % 2).astype(bool)
    runs = ((np.arange(P) // 7) % 2).astype(bool)      # whole voxels go, others lose a head or a tail
    return {"all": np.ones(P, bool), "none": np.zeros(P, bool), "alternating": alt, "alternating'": ~alt,
            "runs": runs, "random": rng.rand(P) < 0.5, "sparse": rng.rand(P) < 0.03}


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "alternating'", "runs", "random", "sparse"])
def test_remap_matches_brute_force(pattern):
    vi, keys, counts, P = _index(3)
    keep = _keeps(P, 4)[pattern]
    reasons = torch.from_numpy((~keep).astype(np.uint8))
    row_map = R.row_map_ref(reasons)
    before = {k: vi.get(k) for k in keys}
    vi.remap(row_map)
    new_row = np.cumsum(keep) - 1                       # new number of a kept row
    lost_all = 0
    for k in keys:
        first, count = before[k]
        rows = [int(new_row[r]) for r in range(first, first + count) if keep[r]]
        got_first, got_count = vi.get(k)
        assert got_count == len(rows), (k, pattern)
        if rows:
            assert rows == list(range(got_first, got_first + got_count)), (k, pattern)   # ONE contiguous run
        else:
            assert 0 <= got_first <= int(keep.sum())
            lost_all += count > 0
    assert len(vi) == len(keys)
    if pattern in ("none", "runs", "sparse"):
        assert lost_all > 0
    # a voxel that lost all its rows is still registered: its key cannot be added again
    for k in keys[:5] + [k for k in keys if before[k][1] and vi.get(k)[1] == 0][:5]:
        with pytest.raises(KeyError):
            vi.add([k], [1], int(keep.sum()))
    assert len(vi) == len(keys)


@pytest.mark.parametrize("pattern", ["alternating", "runs", "random"])
def test_select_after_remap_equals_a_fresh_index(pattern):
    vi, keys, counts, P = _index(7)
    keep = _keeps(P, 8)[pattern]
    row_map = R.row_map_ref(torch.from_numpy((~keep).astype(np.uint8)))
    # the index a model rebuilt from t[keep] would carry: the surviving counts, back to back
    first = np.cumsum([0] + counts[:-1])
    new_counts = [int(keep[f:f + c].sum()) for f, c in zip(first, counts)]
    fresh = G.VoxelIndex()
    assert fresh.add(keys, new_counts, 0) == int(keep.sum())
    vi.remap(row_map)
    for k in keys:
        assert vi.get(k) == fresh.get(k)
    gen = torch.Generator().manual_seed(1)
    picks = [keys[i] for i in torch.randperm(len(keys), generator=gen)[:40].tolist()] + [123456789012]
    losses = {k: torch.randn((3, 3), generator=gen) for k in picks}
    a, b = vi.select(losses), fresh.select(losses)
    assert (a is None) == (b is None) and a is not None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].dtype == torch.int32


def test_remap_accepts_hosts_integers_and_refuses_short_maps():
    vi = G.VoxelIndex()
    vi.add([5, 6, 7], [2, 0, 3], 0)
    with pytest.raises(ValueError):
        vi.remap(torch.tensor([0, 1, 2, 3], dtype=torch.int32))     # 3 rows, the index holds 5
    assert vi.get(7) == (2, 3)                                        # nothing changed
    with pytest.raises(ValueError):
        vi.remap([])
    vi.remap(np.array([0, 0, 1, 1, 2, 3]))                            # keep = 0 1 0 1 1
    assert vi.get(5) == (0, 1) and vi.get(6) == (1, 0) and vi.get(7) == (1, 2)
    vi.remap([0, 1, 2, 3])                                            # nothing dropped
    assert vi.get(5) == (0, 1) and vi.get(6) == (1, 0) and vi.get(7) == (1, 2)
    empty = G.VoxelIndex()
    empty.remap([0])
    assert len(empty) == 0
