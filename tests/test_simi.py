"""CPU tests of the LiDAR similarity loss: the float64 restatement (tests/simi_ref.py), the voxel index and its
selection (gs-livm_amd/model.py) against a literal dict-and-mask transcription of calcSimiLoss
(src/gs/gaussian.cu:201-228, simi_ref.select_by_mask), and the argument checks of the C entry point."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import gs_livm_amd as G
import simi_ref as R


def _index_of(sc):
    vi = G.VoxelIndex()
    assert vi.add(sc["keys"], sc["counts"], 0) == sc["P"]
    return vi


def test_restatement_passes_gradcheck():
    sc = R.make_scene(3, 9, seed=2, spare_voxels=2, empty_voxels=1, unknown_keys=1)
    pts, rows = R.select_by_mask(sc["index"], sc["losses"], sc["P"])
    xyz = torch.from_numpy(sc["xyz"]).double().requires_grad_(True)
    scaling = torch.from_numpy(sc["scaling"]).double().requires_grad_(True)
    fn = lambda x, s: R.similarity_loss_ref(pts.double(), rows, x, s, 0.2)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (xyz, scaling), eps=1e-7, atol=1e-6, rtol=1e-4)
    # the closed form of the contract: lambda/m * sum_i max(min_j d_ij - r, 0)
    with torch.no_grad():
        d = (pts.double()[:, None] - xyz[rows][None]).norm(2, 2).min(1).values
        want = 0.2 * (d - scaling[rows].mean()).clamp(min=0).mean()
    assert abs(float(fn(xyz, scaling).detach()) - float(want)) < 1e-15


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_select_equals_the_mask_transcription(seed):
    sc = R.make_scene(40, 300, seed=seed)
    vi = _index_of(sc)
    want_pts, want_rows = R.select_by_mask(sc["index"], sc["losses"], sc["P"])
    pts, sel = vi.select(sc["losses"])
    assert sel.dtype == torch.int32 and pts.dtype == torch.float32 and pts.shape == (sc["m"], 3)
    assert torch.equal(sel.long(), want_rows) and sel.numel() == sc["n"]
    assert bool((sel[1:] > sel[:-1]).all())                      # ascending, unique
    assert sc["m"] == 300 and sc["m"] < sum(v.shape[0] for v in sc["losses"].values())  # unknown keys dropped points
    # the same points (the order of a hash map's walk is not part of the contract)
    key = lambda t: t[np.lexsort(t.numpy().T[::-1])]  # noqa: E731
    assert torch.equal(key(pts), key(want_pts))
    # the order of `losses` does not matter
    rev = dict(reversed(list(sc["losses"].items())))
    pts2, sel2 = vi.select(rev)
    assert torch.equal(pts2, pts) and torch.equal(sel2, sel)


def test_empty_voxels_unknown_keys_and_duplicates():
    vi = G.VoxelIndex()
    assert vi.add([10, 11, 12, 13], [2, 0, 3, 0], 5) == 10
    assert vi.get(10) == (5, 2) and vi.get(11) == (7, 0) and vi.get(12) == (7, 3) and 13 in vi and 99 not in vi
    assert len(vi) == 4
    with pytest.raises(KeyError):
        vi.add([14, 12], [1, 1], 10)     # 12 is known: nothing is registered, 14 included
    assert 14 not in vi and len(vi) == 4
    with pytest.raises(KeyError):
        vi.add([20, 20], [1, 1], 10)
    assert 20 not in vi
    with pytest.raises(ValueError):
        vi.add([30], [1, 2], 10)
    p = lambda k: torch.arange(3 * k, dtype=torch.float32).reshape(k, 3)  # noqa: E731
    assert vi.select({99: p(4)}) is None                       # nothing matches
    assert vi.select({}) is None
    assert vi.select({10: p(0)}) is None                       # a known key without points: no point is left
    assert vi.select({11: p(2), 13: p(1)}) is None             # points, but only empty voxels: nothing to compare with
    pts, sel = vi.select({99: p(4), 12: p(2), 11: p(1)})
    assert sel.tolist() == [7, 8, 9] and pts.shape == (3, 3)   # the empty voxel's point stays, key 99's are dropped
    pts, sel = vi.select({12: p(1), 10: p(1)})
    assert sel.tolist() == [5, 6, 7, 8, 9]
    # overlapping ranges (two indices merged by hand) still give unique ascending rows
    vj = G.VoxelIndex()
    vj.add([1], [4], 0)
    vj.add([2], [4], 2)
    assert vj.select({1: p(1), 2: p(1)})[1].tolist() == [0, 1, 2, 3, 4, 5]


def test_subsample_499_keeps_all_500_keeps_exactly_500():
    vi = G.VoxelIndex()
    vi.add([1, 2], [16, 16], 0)
    gen = torch.Generator().manual_seed(7)
    cloud = torch.randn((700, 3), generator=gen)
    pts, _ = vi.select({1: cloud[:250], 2: cloud[250:499]})
    assert torch.equal(pts, cloud[:499])
    for total in (500, 700):
        losses = {1: cloud[:250], 2: cloud[250:total]}
        a, _ = vi.select(losses, generator=torch.Generator().manual_seed(3))
        b, _ = vi.select(losses, generator=torch.Generator().manual_seed(3))
        c, _ = vi.select(losses, generator=torch.Generator().manual_seed(4))
        assert a.shape == (500, 3) and torch.equal(a, b) and not torch.equal(a, c)
        want = cloud[:total].index_select(0, torch.randperm(total, generator=torch.Generator().manual_seed(3))[:500])
        assert torch.equal(a, want)                              # randperm + slice, as the reference draws it
        assert len({tuple(r) for r in a.tolist()}) == 500        # a subset: no point twice
    pts, _ = vi.select({1: cloud[:250], 2: cloud[250:]}, max_points=100, generator=torch.Generator().manual_seed(1))
    assert pts.shape == (100, 3)


def test_add_new_pointcloud_signature_keeps_its_old_form():
    """The first four parameters and their defaults are what they were; the index arguments are optional, come after
    them and default to None.  (That the rows come out the same is tests/test_gpu_growth.py's business.)"""
    sig = inspect.signature(G.GrowableGaussians.add_new_pointcloud)
    names = list(sig.parameters)
    assert names[:5] == ["self", "xyz", "covs", "rgbs", "scale_factor"] and sig.parameters["scale_factor"].default == 1.0
    assert names[5:] == ["voxel_keys", "voxel_counts"]
    assert sig.parameters["voxel_keys"].default is None and sig.parameters["voxel_counts"].default is None


def test_add_new_pointcloud_checks_the_index_arguments_before_it_changes_anything():
    m = G.GrowableGaussians.__new__(G.GrowableGaussians)   # (no device buffers: the checks come first)
    m.P, m.voxel_index = 7, G.VoxelIndex()
    z = torch.zeros
    with pytest.raises(ValueError):
        m.add_new_pointcloud(z(4, 3), z(4, 3, 3), z(4, 3), voxel_keys=[1, 2], voxel_counts=[1, 2])   # 3 != 4
    with pytest.raises(ValueError):
        m.add_new_pointcloud(z(4, 3), z(4, 3, 3), z(4, 3), voxel_keys=[1, 2])
    with pytest.raises(KeyError):
        m.add_new_pointcloud(z(4, 3), z(4, 3, 3), z(4, 3), voxel_keys=[1, 1], voxel_counts=[2, 2])
    assert len(m.voxel_index) == 0 and m.P == 7
    # no rows, keys only: voxels whose sample was empty are registered and nothing else happens
    assert m.add_new_pointcloud(z(0, 3), z(0, 3, 3), z(0, 3), voxel_keys=[5, 6], voxel_counts=[0, 0]) == (7, 7)
    assert m.voxel_index.get(5) == (7, 0) and m.voxel_index.get(6) == (7, 0)
    assert m.add_new_pointcloud(z(0, 3), z(0, 3, 3), z(0, 3)) == (7, 7) and len(m.voxel_index) == 2


def test_similarity_loss_argument_errors_are_reported_not_crashed():
    L = G.lib()
    assert "gsr_similarity_loss" in G._capi.EXPORTS and "gsr_similarity_loss_workspace" in G._capi.EXPORTS
    ws = L.gsr_similarity_loss_workspace
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0
    prev = 0
    for m, n in ((1, 1), (7, 16), (500, 8000), (500, 32000), (3000, 50000)):
        b = ws(m, n)
        assert b >= max(prev, 16 * m) and b % 256 == 0 and b < (64 << 20)
        prev = b
    assert ws(1 << 20, 1 << 24) < (1 << 20) * 64   # bounded by the points, not by m * n
    null = C.c_void_p(None)
    fake = C.c_void_p(256)  # never dereferenced: every call below fails its checks before any device work
    call = lambda P, m, n, pts=fake, sel=fake, xyz=fake, sc=fake, out=fake, w=fake, wb=1 << 30: \
        L.gsr_similarity_loss(P, m, n, pts, sel, xyz, sc, 0.2, out, null, null, 0, w, wb, null)  # noqa: E731
    err = lambda: L.gsr_last_error().decode()  # noqa: E731
    assert call(-1, 1, 1) < 0 and "bad" in err()
    assert call(10, -1, 1) < 0 and call(10, 1, -1) < 0
    assert call(4, 3, 5) < 0 and "selected rows" in err()         # more unique rows than the model has
    assert call(10, 3, 5, out=null) < 0 and "null" in err()
    for k in ("pts", "sel", "xyz", "sc", "w"):
        assert call(10, 3, 5, **{k: null}) < 0 and "null" in err(), k
    assert call(10, 3, 5, wb=ws(3, 5) - 1) < 0 and "workspace too small" in err()
    assert call(10, 0, 0, out=null) < 0                            # out3 is needed even when there is no term
