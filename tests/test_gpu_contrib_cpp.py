"""GPU tests of the C++/LibTorch route of the per-Gaussian blend contribution (csrc/torch_next.cpp: contribution,
contribution_finish) against the Python route (gs-livm_amd/contribution.py over _capi).  Both launch the same kernels with
the same arguments: results must be bit-identical."""
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S

from helpers import hip_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx(gpu_device):
    return G.torch_ops().next


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_rows_and_outputs_match_the_python_route(nx, gpu_device):
    dev = gpu_device
    P, W, H = 2500, 257, 131
    sc = S.make_scene(P, W, H, 4, sh_degree=2)
    _, fwd = hip_forward(sc, dev, debug=False)
    stats_py, stats_cpp = torch.zeros((P, 3), device=dev), torch.zeros((P, 3), device=dev)
    y = G.contribution(fwd, P, W, H, min_pixels=3, min_weight=0.01, stats=stats_py)
    rows = nx.contribution(fwd[5], fwd[6], fwd[7], P, G._capi._key(fwd[0]), W, H)
    assert y.rows.any() and _same(rows, y.rows)
    x = nx.contribution_finish(rows, 3, 0.01, stats=stats_cpp)
    for a, b in zip(x, (y.n_touched, y.weight_sum, y.weight_max, y.mask)):
        assert _same(a, b)
    assert stats_py.any() and _same(stats_cpp, stats_py)
    assert 0 < int(y.mask.sum()) < int((y.n_touched > 0).sum())      # the thresholds bite
    x = nx.contribution_finish(rows, want_n_touched=False, want_weight_max=False)
    assert x[0] is None and x[2] is None and _same(x[1], y.weight_sum)
    assert _same(x[3], (y.n_touched >= 1).to(torch.uint8))


def test_an_empty_model(nx, gpu_device):
    e = torch.empty(0, dtype=torch.uint8, device=gpu_device)
    rows = nx.contribution(e, e, e, 0, 0, 33, 17)
    assert rows.shape == (0, 2) and rows.dtype == torch.int64
    x = nx.contribution_finish(rows)
    assert all(t is not None and t.numel() == 0 for t in x)
