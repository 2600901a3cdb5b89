"""CPU tests of the argument validation of gsr_sweep_admit and gsr_sweep_admit_workspace (no device involved:
validation comes first), at the C entry point and through gs_livm_amd._capi."""
import ctypes as C
import math
import re

import pytest
import torch

import gs_livm_amd as G

ONE = C.c_void_p(256)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
F9 = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
F12 = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
INF = float("inf")


def _admit(L, n=5, H=16, W=16, T=F12, K=F9, lo=0.2, hi=INF, acc_min=0.5, depth_tol=0.05, radius=1, occlusion_tol=0.1,
           footprint=1.0, short=0, ws=ONE, **ptrs):
    p = dict(points=ONE, covs=NULL, depth=NULL, acc=NULL, lidar=NULL, image=NULL, exposure=NULL, xyz=ONE, covs_out=ONE,
             rgb=NULL, index=ONE, pixel=NULL, z=NULL, reasons=NULL, counts=ONE)
    p.update(ptrs)
    nbytes = max(int(L.gsr_sweep_admit_workspace(n, H, W)) - short, 0)
    return L.gsr_sweep_admit(n, p["points"], p["covs"], T, K, H, W, lo, hi, p["depth"], p["acc"], acc_min, depth_tol,
                             p["lidar"], radius, occlusion_tol, p["image"], p["exposure"], footprint, 1, p["xyz"],
                             p["covs_out"], p["rgb"], p["index"], p["pixel"], p["z"], p["reasons"], p["counts"], ws,
                             nbytes, NULL)


def test_symbols_are_exported_and_the_abi_version_stays():
    for s in ("gsr_sweep_admit", "gsr_sweep_admit_workspace"):
        assert s in G._capi.EXPORTS and hasattr(G.lib(), s)
    assert G.lib().gsr_abi_version() == 2
    # no kernel id was added: the profiler's mask is full, the launches are timed under k_visibility
    names = [G.lib().gsr_kernel_name(i).decode() for i in range(G.lib().gsr_kernel_count())]
    assert "k_visibility" in names and not any("seed" in k for k in names) and len(names) <= 64
    assert callable(G.admit_sweep) and G.Admitted._fields == ("xyz", "covs", "rgbs", "index", "pixel", "z", "counts",
                                                              "reasons")
    assert hasattr(G.GrowableGaussians, "add_unexplained")


def test_shapes_are_refused_and_their_workspace_is_zero():
    L = G.lib()
    err = L.gsr_last_error
    assert _admit(L, n=-1) == -1 and b"bad n" in err()
    assert L.gsr_sweep_admit_workspace(-1, 16, 16) == 0
    for H, W in ((0, 16), (16, 0), (-3, 16), (16, -3)):
        assert _admit(L, H=H, W=W) == -1 and b"bad image shape" in err(), (H, W)
        assert L.gsr_sweep_admit_workspace(5, H, W) == 0
    for H, W in ((65536, 32768), (2, 1 << 30), (46341, 46341)):      # H W >= 2^31
        assert H * W >= 2 ** 31
        assert _admit(L, H=H, W=W) == -1 and b"too large" in err(), (H, W)
        assert L.gsr_sweep_admit_workspace(5, H, W) == 0
    assert L.gsr_sweep_admit_workspace(5, 1, 1) > 0 and L.gsr_sweep_admit_workspace(1, 46340, 46340) > 8 * 46340 ** 2
    assert L.gsr_sweep_admit_workspace(0, 16, 16) == 0                # n == 0 needs none


def test_null_pointers_and_the_render_pair_are_refused():
    L = G.lib()
    err = L.gsr_last_error
    for name in ("points", "xyz", "covs_out", "index", "counts"):
        assert _admit(L, **{name: NULL}) == -1 and b"null pointer" in err(), name
    assert _admit(L, T=None) == -1 and b"null pointer" in err()
    assert _admit(L, K=None) == -1 and b"null pointer" in err()
    assert _admit(L, ws=NULL) == -1 and b"null pointer" in err()
    assert _admit(L, depth=ONE) == -1 and b"depth and acc" in err()
    assert _admit(L, acc=ONE) == -1 and b"depth and acc" in err()
    assert _admit(L, points=C.c_void_p(258)) == -1 and b"misaligned" in err()


def test_scalars_are_refused():
    L = G.lib()
    err = L.gsr_last_error
    for a in (0.0, -0.5, INF, math.nan):
        assert _admit(L, acc_min=a) == -1 and b"bad acc_min" in err(), a
    for name in ("depth_tol", "occlusion_tol", "footprint"):
        for v in (-0.1, INF, -INF, math.nan):
            assert _admit(L, **{name: v}) == -1 and ("bad " + name).encode() in err(), (name, v)
    for r in (-1, 4, 100):
        assert _admit(L, radius=r) == -1 and b"bad occlusion_radius" in err(), r
    for lo in (-0.1, INF, math.nan):
        assert _admit(L, lo=lo) == -1 and b"bad min_depth" in err(), lo
    for lo, hi in ((0.2, 0.2), (0.2, 0.1), (0.0, 0.0), (0.2, math.nan), (0.2, -INF)):
        assert _admit(L, lo=lo, hi=hi) == -1 and b"bad max_depth" in err(), (lo, hi)


def test_a_short_workspace_is_refused_and_the_message_names_the_bytes():
    L = G.lib()
    need = int(L.gsr_sweep_admit_workspace(5, 16, 16))
    assert _admit(L, short=1) == -1
    msg = L.gsr_last_error().decode()
    assert "workspace too small" in msg and int(re.search(r"need (\d+) bytes", msg).group(1)) == need
    assert need >= 8 * 16 * 16 + 6 * 4 + 5


def test_the_order_of_the_checks():
    L = G.lib()
    err = L.gsr_last_error
    assert _admit(L, n=-1, H=0, points=NULL) == -1 and b"bad n" in err()
    assert _admit(L, H=0, points=NULL, acc_min=0.0) == -1 and b"bad image shape" in err()
    assert _admit(L, xyz=NULL, depth=ONE) == -1 and b"null pointer" in err()
    assert _admit(L, depth=ONE, acc_min=0.0) == -1 and b"depth and acc" in err()
    assert _admit(L, acc_min=0.0, depth_tol=-1.0) == -1 and b"bad acc_min" in err()
    assert _admit(L, depth_tol=-1.0, radius=9) == -1 and b"bad depth_tol" in err()
    assert _admit(L, radius=9, lo=-1.0) == -1 and b"bad occlusion_radius" in err()
    assert _admit(L, lo=-1.0, short=1) == -1 and b"bad min_depth" in err()


def test_capi_raises_on_a_refusal():
    """Through gs_livm_amd._capi: the refusals surface as GsrError before any device work.  (The tensors would have to
    live on a device, so the wrapper's own assertions come first on a machine without one; the C message is what a
    device caller sees.)"""
    with pytest.raises((G.GsrError, AssertionError)):
        G._capi.sweep_admit(torch.zeros((4, 3)), torch.eye(4), torch.eye(3), 16, 16, -1.0, 0.1)
    with pytest.raises(TypeError):
        G.admit_sweep(torch.zeros((4, 3)), torch.eye(4), torch.eye(3), 16, 16)     # the tolerances have no default
