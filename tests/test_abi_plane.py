"""CPU tests of the argument validation of gsr_surfel_plane_loss and gsr_surfel_plane_loss_workspace (no device
involved: validation comes first), at the C entry point and through gs_livm_amd._capi."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import gs_livm_amd as G

ONE = C.c_void_p(256)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
INF = float("inf")
KERNELS_BEFORE = 64


def _loss(L, P=100, m=5, n=4, lam=0.2, huber=0.02, max_dist=0.05, lambda_flat=0.3, short=0, ws=ONE, out4=ONE, **ptrs):
    p = dict(points=ONE, sel=ONE, xyz=ONE, scaling=ONE, rotation=ONE, grad_xyz=NULL, grad_scaling=NULL,
             grad_rotation=NULL)
    p.update(ptrs)
    nbytes = max(int(L.gsr_surfel_plane_loss_workspace(m, n)) - short, 0)
    return L.gsr_surfel_plane_loss(P, m, n, p["points"], p["sel"], p["xyz"], p["scaling"], p["rotation"], lam, huber,
                                   max_dist, lambda_flat, out4, p["grad_xyz"], p["grad_scaling"], p["grad_rotation"],
                                   0, ws, nbytes, NULL)


def test_symbols_are_exported_and_neither_the_abi_version_nor_the_kernel_table_moves():
    L = G.lib()
    for s in ("gsr_surfel_plane_loss", "gsr_surfel_plane_loss_workspace"):
        assert s in G._capi.EXPORTS and hasattr(L, s)
    assert L.gsr_abi_version() == 2
    # no kernel id was added (the profiler's mask is full): the launches are timed under the similarity loss's three
    assert L.gsr_kernel_count() == KERNELS_BEFORE
    names = [L.gsr_kernel_name(i).decode() for i in range(KERNELS_BEFORE)]
    assert len(set(names)) == KERNELS_BEFORE and not any("surfel" in k or "plane" in k for k in names)
    assert {"k_simi_nearest", "k_simi_points", "k_simi_grads"} <= set(names)
    assert callable(G.surfel_plane_loss) and issubclass(G.SurfelPlaneLoss, torch.autograd.Function)
    assert hasattr(G.GrowableGaussians, "calc_plane_loss")


def test_the_kernel_names_are_the_64_on_record():
    """The table as the parent commit had it, name by name (kept in tests/golden/kernel_names_64.txt)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names_64.txt")
    want = open(path).read().split()
    L = G.lib()
    assert len(want) == KERNELS_BEFORE
    assert [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())] == want


def test_the_workspace_query():
    q = G.lib().gsr_surfel_plane_loss_workspace
    for m, n in ((0, 4), (4, 0), (-1, 4), (4, -1), (0, 0), (4, 0x7fffffff - 1023), (4, 0x7fffffff)):
        assert q(m, n) == 0, (m, n)
    sizes = [int(q(m, 8000)) for m in (1, 500, 3000, 100000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4
    assert sizes[3] >= 100000 * (8 + 20)          # one partial (distance, position) and one 20-byte record per point
    assert int(q(500, 50000)) >= int(q(500, 16)) + 4 * 50000 - 4 * 16     # k* per selected row


def test_every_refusal_in_its_order_with_a_message():
    L = G.lib()
    err = L.gsr_last_error
    bad = -1
    # 1. negative P, m, n
    for kw in (dict(P=-1), dict(m=-1), dict(n=-1)):
        assert _loss(L, **kw) == bad and b"bad P/m/n" in err(), kw
    # 2. n > P   3. n beyond the similarity loss's bound
    assert _loss(L, P=3, n=4) == bad and b"selected rows" in err()
    assert _loss(L, P=0x7fffffff, n=0x7fffffff - 1023) == bad and b"n too large" in err()
    assert G.lib().gsr_similarity_loss(0x7fffffff, 5, 0x7fffffff - 1023, ONE, ONE, ONE, ONE, 0.2, ONE, NULL, NULL, 0,
                                       ONE, 0, NULL) == bad and b"n too large" in err()       # (the same bound)
    # 4. lambda, huber, lambda_flat: finite and >= 0
    for name in ("lam", "huber", "lambda_flat"):
        for v in (-0.1, INF, -INF, math.nan):
            what = ("bad " + {"lam": "lambda"}.get(name, name)).encode()
            assert _loss(L, **{name: v}) == bad and what in err(), (name, v)
        assert _loss(L, **{name: 0.0}, points=NULL) == bad and b"null pointer" in err()      # 0 is legal
    # 5. max_dist: not NaN, > 0; +inf is legal
    for v in (0.0, -1.0, -INF, math.nan):
        assert _loss(L, max_dist=v) == bad and b"bad max_dist" in err(), v
    assert _loss(L, max_dist=INF, points=NULL) == bad and b"null pointer" in err()
    # 6. out4   7. required inputs and the workspace, with m, n > 0
    assert _loss(L, out4=NULL) == bad and b"null pointer" in err()
    for name in ("points", "sel", "xyz", "scaling", "rotation"):
        assert _loss(L, **{name: NULL}) == bad and b"null pointer" in err(), name
    assert _loss(L, ws=NULL) == bad and b"null pointer" in err()
    # 8. the workspace size, by its number
    need = int(L.gsr_surfel_plane_loss_workspace(5, 4))
    assert _loss(L, short=1) == bad
    msg = err().decode()
    assert "workspace too small" in msg and int(re.search(r"need (\d+) bytes", msg).group(1)) == need
    # 9. alignment of every float / int array
    for name in ("points", "sel", "xyz", "scaling", "rotation", "grad_xyz", "grad_scaling", "grad_rotation"):
        for off in (1, 2, 3):
            assert _loss(L, **{name: C.c_void_p(256 + off)}) == bad and b"misaligned" in err(), (name, off)
    assert _loss(L, out4=C.c_void_p(258)) == bad and b"misaligned" in err()
    # the order: each refusal wins over all that follow it
    chain = [(dict(m=-1), b"bad P/m/n"), (dict(P=3, n=4), b"selected rows"), (dict(lam=-1.0), b"bad lambda"),
             (dict(huber=math.nan), b"bad huber"), (dict(lambda_flat=INF), b"bad lambda_flat"),
             (dict(max_dist=0.0), b"bad max_dist"), (dict(out4=NULL), b"null pointer"),
             (dict(rotation=NULL), b"null pointer"), (dict(short=1), b"workspace too small"),
             (dict(xyz=C.c_void_p(258)), b"misaligned")]
    for i, (kw, what) in enumerate(chain):
        later = {}
        for kw2, _ in chain[i + 1:]:
            later.update(kw2)
        later.update(kw)
        assert _loss(L, **later) == bad and what in err(), (i, err())


def test_a_refusal_writes_nothing():
    """Host buffers stand in for the device's (nothing dereferences them before a refusal): every byte stays."""
    L = G.lib()
    bufs = {k: np.full(64, 0x5A, np.uint8) for k in ("out4", "grad_xyz", "grad_scaling", "grad_rotation", "ws")}
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    kw = dict(out4=ptr["out4"], ws=ptr["ws"], grad_xyz=ptr["grad_xyz"], grad_scaling=ptr["grad_scaling"],
              grad_rotation=ptr["grad_rotation"])
    for refuse in (dict(m=-1), dict(P=3, n=4), dict(lam=math.nan), dict(huber=-1.0), dict(lambda_flat=-1.0),
                   dict(max_dist=math.nan), dict(points=NULL), dict(short=1), dict(sel=C.c_void_p(257))):
        assert _loss(L, **{**kw, **refuse}) == -1, refuse
        assert L.gsr_last_error() != b""
        assert all(bool((v == 0x5A).all()) for v in bufs.values()), refuse


def test_capi_and_the_python_surface():
    with pytest.raises((G.GsrError, AssertionError)):
        G._capi.surfel_plane_loss(torch.zeros((4, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((8, 3)),
                                  torch.ones((8, 3)), torch.ones((8, 4)), -1.0)
    with pytest.raises(TypeError):
        G.surfel_plane_loss(torch.zeros((4, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((8, 3)),
                            torch.ones((8, 3)), torch.ones((8, 4)))           # lambda_ has no default
    import inspect
    sig = inspect.signature(G.GrowableGaussians.calc_plane_loss)
    assert list(sig.parameters)[1:] == ["losses", "lambda_", "scaling", "rotation", "huber", "max_dist", "lambda_flat",
                                        "max_points", "generator"]
    assert sig.parameters["lambda_"].default is inspect.Parameter.empty and sig.parameters["max_points"].default == 500
