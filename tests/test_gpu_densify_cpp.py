"""GPU tests of the C++/LibTorch route of adaptive density control (csrc/torch_next.cpp: density_accumulate,
densify_mark, densify_apply) against the Python route (gs-livm_amd/_capi.py).  Both launch the same kernels with the
same arguments: results must be bit-identical, as in test_gpu_prune_cpp.py."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

import densify_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx(gpu_device):
    return G.torch_ops().next


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def test_accumulate_and_mark_match_the_python_route(nx, gpu_device):
    dev, P = gpu_device, 1025
    views, stats0, _ = Cs.accumulate_case(P)
    a, b = torch.from_numpy(stats0).to(dev), torch.from_numpy(stats0).to(dev)
    for radii, g in views:
        r, g = torch.from_numpy(radii).to(dev), torch.from_numpy(g).to(dev)
        nx.density_accumulate(r, g, a)
        _capi.density_accumulate(r, g, b)
    assert _same(a, b) and bool((b[:, 1] > 0).any())
    stats, scaling, cand = Cs.mark_case(P, "0.5")
    st, sc = torch.from_numpy(stats).to(dev), torch.from_numpy(scaling).to(dev)
    for max_new in (None, 0, 100):
        x = nx.densify_mark(st, sc, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD, -1 if max_new is None else max_new)
        y = _capi.densify_mark(st, sc, Cs.GRAD_THRESHOLD, Cs.SIZE_THRESHOLD, max_new)
        for s, t in zip(x, y):
            assert _same(s, t)
        assert int(x[2][0]) == (int(cand.sum()) if max_new is None else max_new)


@pytest.mark.parametrize("P,M", [(300, 4), (257, 1)])
def test_apply_matches_the_python_route(P, M, nx, gpu_device):
    dev = gpu_device
    leaves, moments, stats, kinds, offs = Cs.apply_case(P, M)
    n_new = int(offs[-1])

    def buffers(arrays):
        out = []
        for a in arrays:
            t = torch.full((P + n_new + 3,) + a.shape[1:], float("nan"), device=dev)
            t[:P] = torch.from_numpy(a).to(dev)
            out.append(t)
        return out
    k, o = torch.from_numpy(kinds).to(dev), torch.from_numpy(offs).to(dev)
    for with_state in (True, False):
        pa, pb = buffers(leaves), buffers(leaves)
        ma, mb, va, vb = buffers(moments[:6]), buffers(moments[:6]), buffers(moments[6:]), buffers(moments[6:])
        (sa,), (sb,) = buffers([stats]), buffers([stats])
        if with_state:
            nx.densify_apply(P, n_new, k, o, 77, pa, ma, va, sa)
            _capi.densify_apply(P, n_new, k, o, 77, pb, mb, vb, sb)
        else:
            nx.densify_apply(P, n_new, k, o, 77, pa)
            _capi.densify_apply(P, n_new, k, o, 77, pb)
        for x, y in zip(pa + ma + va + [sa], pb + mb + vb + [sb]):
            assert _same(x, y)
        assert bool(torch.isfinite(pb[0][:P + n_new]).all()) and bool(torch.isnan(pb[0][P + n_new:]).all())
        assert bool(torch.isnan(mb[0][P:P + n_new]).all()) != with_state     # moments are written only when handed over
    # a buffer with fewer than P + n_new rows is refused on the host, on both routes
    short = [t[:P + n_new - 1] if t.numel() else t for t in pa]
    with pytest.raises(Exception):
        nx.densify_apply(P, n_new, k, o, 77, short)
    with pytest.raises(AssertionError):
        _capi.densify_apply(P, n_new, k, o, 77, short)
    assert np.isfinite(pa[0][:P + n_new].cpu().numpy()).all()
