"""GPU tests of the C++/LibTorch route of the normal-map feature (csrc/torch_next.cpp: blend_attributes, surfel_normals,
normal_consistency_loss) against the Python route (gs-livm_amd/normals.py over _capi).  Both launch the same kernels with
the same arguments: results must be bit-identical."""
import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S

import normal_ref as NR
from helpers import hip_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nx(gpu_device):
    return G.torch_ops().next


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_blend_matches_the_python_route(nx, gpu_device):
    dev = gpu_device
    P, W, H = 2500, 257, 131
    sc = S.make_scene(P, W, H, 4, sh_degree=2)
    _, fwd = hip_forward(sc, dev, debug=False)
    for C in (1, 3, 4):
        at = torch.randn((P, C), generator=torch.Generator().manual_seed(C)).to(dev)
        y = G.blend_attributes(fwd, at, W, H)
        x = nx.blend_attributes(fwd[5], fwd[6], fwd[7], at, G._capi._key(fwd[0]), W, H)
        assert y.any() and _same(x, y)
    e = torch.empty(0, dtype=torch.uint8, device=dev)
    x = nx.blend_attributes(e, e, e, torch.empty((0, 2), device=dev), 0, 33, 17)
    assert x.shape == (2, 17, 33) and not x.any()


def test_normals_match_the_python_route(nx, gpu_device):
    xyz, s, q, T = (torch.from_numpy(a) for a in NR.normal_rows())
    xyz, s, q = xyz.to(gpu_device), s.to(gpu_device), q.to(gpu_device)
    y = G.surfel_normals(xyz, s, q, T)
    assert y.any() and _same(nx.surfel_normals(xyz, s, q, T), y)
    assert nx.surfel_normals(xyz[:0], s[:0], q[:0], T).shape == (0, 3)


def test_loss_and_gradients_match_the_python_route(nx, gpu_device):
    dev = gpu_device
    W, H = 37, 23
    D, A, N, cam = NR.loss_case(W, H)
    K = torch.tensor([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], dtype=torch.float64)
    res = []
    for route in ("py", "cpp"):
        d = torch.from_numpy(D).to(dev).requires_grad_(True)
        a = torch.from_numpy(A).to(dev).requires_grad_(True)
        n = torch.from_numpy(N).to(dev)
        if route == "py":
            loss = G.normal_consistency_loss(d, a, n, K, 0.5, lambda_=0.7, normal_min=0.1, jump_rel=0.05)
        else:
            loss = nx.normal_consistency_loss(d, a, n, K, 0.5, 0.7, 0.1, 0.05)
        (loss * 0.25).backward()
        res.append((loss.detach(), d.grad, a.grad))
    assert float(res[0][0]) > 0 and res[0][1].any() and res[0][2].any()
    for x, y in zip(*res):
        assert _same(x, y)
    # only depth asks for a gradient
    d = torch.from_numpy(D).to(dev).requires_grad_(True)
    a = torch.from_numpy(A).to(dev)
    nx.normal_consistency_loss(d, a, torch.from_numpy(N).to(dev), K, 0.5, 0.7, 0.1).backward()
    assert d.grad is not None and a.grad is None
    assert np.isfinite(d.grad.cpu().numpy()).all()
