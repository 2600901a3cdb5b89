"""GPU tests of the C++/LibTorch route of in-place pruning (csrc/torch_next.cpp: prune_mark, prune_rows,
FusedAdam::prune, VoxelIndex::remap) against the Python route (gs-livm_amd/_capi.py, model.py).  Both launch the same
kernels with the same arguments: results must be bit-identical, as in test_gpu_next_cpp.py."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import prune_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx(gpu_device):
    return G.torch_ops().next


def _leaves(P, M, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    L = dict(xyz=r(P, 3), fdc=r(P, 1, 3), frest=r(P, M - 1, 3) * 0.1, scaling=r(P, 3) * 0.3 - 3.0, rotation=r(P, 4),
             opacity=r(P, 1))
    dead = torch.rand(P, generator=gen).to(dev) < 0.4
    even = torch.arange(P, device=dev) % 2 == 0
    L["scaling"][dead & even, 2] = 0.7
    L["opacity"][dead & ~even] = -9.0
    L["xyz"][5, 0] = float("nan")
    return L


@pytest.mark.parametrize("M", [1, 4])
def test_mark_rows_and_optimizer_match_the_python_route(M, nx, gpu_device):
    dev, P = gpu_device, 10_007
    L = _leaves(P, M, dev, seed=M)
    mask = torch.rand(P, device=dev) < 0.1
    for kw in (dict(), dict(min_opacity=0.3, max_scale=0.06, drop_nonfinite=False, drop=mask)):
        a = nx.prune_mark(L["xyz"], L["scaling"], L["rotation"], L["opacity"], **kw)
        b = _capi.prune_mark(L["xyz"], L["scaling"], L["rotation"], L["opacity"], **kw)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
        assert a[2].tolist() == R.counts_ref(a[0]) and 0 < int(a[2][0]) < P
    reasons, row_map, counts = a
    P_new = int(counts[0])
    order = ("xyz", "fdc", "frest", "scaling", "rotation", "opacity")
    lrs = [0.0005, 0.001, 0.001 / 20.0, 0.0025, 0.0025, 0.025]
    params = [L[k].clone().requires_grad_(True) for k in order]
    opt = nx.FusedAdam(params, lrs, 0.9, 0.999, 1e-15)
    gen = torch.Generator().manual_seed(9)
    for it in range(2):     # non-zero moments, step count 2
        g_act = [torch.randn(s, generator=gen).to(dev) for s in ((P, 3), (P, 3), (P, 4), (P, 1), (P, M, 3))]
        opt.step_model(*g_act)
    old = [t.detach().clone() for t in list(opt.params()) + list(opt.exp_avg()) + list(opt.exp_avg_sq())]
    want = G.prune_rows(old, reasons, row_map, P_new)                 # the Python route, eighteen tensors
    for x, y in zip(nx.prune_rows(old, reasons, row_map, P_new), want):
        assert x.shape == y.shape and torch.equal(x, y)
    for x, y in zip(want, R.compact_ref(old, reasons)):
        assert torch.equal(x, y)
    opt.prune(reasons, row_map, P_new)
    got = list(opt.params()) + list(opt.exp_avg()) + list(opt.exp_avg_sq())
    for x, y in zip(got, want):
        assert x.shape == y.shape and torch.equal(x.detach(), y)
    assert opt.step_count() == 2 and all(p.requires_grad and p.is_leaf for p in opt.params())
    # it steps on: the next step equals the Python kernel call on the compacted tensors
    ref_p, ref_m, ref_v = ([t.clone() for t in want[i:i + 6]] for i in (0, 6, 12))
    g_act = [torch.randn(s, generator=gen).to(dev) for s in ((P_new, 3), (P_new, 3), (P_new, 4), (P_new, 1), (P_new, M, 3))]
    expect = _capi.model_step(ref_p, ref_m, ref_v, *g_act, lrs, 0.9, 0.999, 1e-15, 3)
    for x, y in zip(opt.step_model(*g_act), expect):
        assert torch.equal(x, y)
    for x, y in zip(opt.params(), ref_p):
        assert torch.equal(x.detach(), y)


def test_voxel_index_remap_matches_the_python_route(nx, gpu_device):
    rng = np.random.RandomState(1)
    counts = rng.randint(0, 9, size=200)
    counts[::7] = 0
    keys = (rng.permutation(10_000)[:200] * 13 + 1).tolist()
    P = int(counts.sum())
    a, b = nx.VoxelIndex(), G.VoxelIndex()
    assert a.add(keys, counts.tolist(), 0) == b.add(keys, counts.tolist(), 0) == P
    keep = torch.from_numpy(rng.rand(P) < 0.4)
    keep[:40] = False
    row_map = R.row_map_ref((~keep).to(torch.uint8))
    a.remap(row_map)
    b.remap(row_map)
    for k in keys:
        assert tuple(a.get(k)) == tuple(b.get(k))
    assert a.get(123) is None and len(a) == len(b) == 200
    with pytest.raises(Exception):
        a.add([keys[0]], [1], int(keep.sum()))            # emptied (its first 40 rows went) yet still registered
    with pytest.raises(Exception):
        a.remap(row_map[:10])
    losses = {k: torch.randn(2, 3) for k in keys[::5]}
    pa, pb = a.select(losses, 500, "cuda"), b.select(losses)
    pb = (pb[0].to(gpu_device), pb[1].to(gpu_device))
    assert torch.equal(pa[0].to(gpu_device), pb[0]) and torch.equal(pa[1].to(gpu_device), pb[1])
