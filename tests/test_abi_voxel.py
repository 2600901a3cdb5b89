"""CPU tests of the argument validation of gsr_voxel_sweep, gsr_voxel_rehash and their two size queries (no device
involved: validation comes first), at the C entry point and through gs_livm_amd._capi."""
import ctypes as C
import math

import pytest
import torch

import gs_livm_amd as G

ONE = C.c_void_p(256)   # never dereferenced: validation fails first
NULL = C.c_void_p(None)
INF = float("inf")
NAMES = ("points", "colors", "table", "status", "point_keys", "xyz", "covs", "rgb", "keys", "npoints", "scaling",
         "rotation", "normal", "counts")


def _sweep(L, n=5, grid=0.2, min_points=10, min_sigma=0.001, sf=1.0, capacity=64, live=0, short=0, ws=ONE, **ptrs):
    p = {k: ONE for k in NAMES}
    p.update(colors=NULL, rgb=NULL)
    p.update(ptrs)
    nbytes = max(int(L.gsr_voxel_sweep_workspace(n)) - short, 0)
    return L.gsr_voxel_sweep(n, p["points"], p["colors"], grid, min_points, min_sigma, sf, p["table"], capacity, live,
                             p["status"], p["point_keys"], p["xyz"], p["covs"], p["rgb"], p["keys"], p["npoints"],
                             p["scaling"], p["rotation"], p["normal"], p["counts"], ws, nbytes, NULL)


def test_symbols_python_names_and_no_new_kernel_id():
    L = G.lib()
    for s in ("gsr_voxel_table_bytes", "gsr_voxel_sweep_workspace", "gsr_voxel_sweep", "gsr_voxel_rehash"):
        assert s in G._capi.EXPORTS and hasattr(L, s)
    assert L.gsr_abi_version() == 2
    # no kernel id was added: the profiler's mask is full, the launches are timed under k_visibility
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    assert "k_visibility" in names and not any("voxel" in k for k in names) and len(names) <= 64
    for n in ("SweepVoxelMap", "VoxelSeeds"):
        assert n in G.__all__ and hasattr(G, n)
    assert G.VoxelSeeds._fields == ("xyz", "covs", "rgbs", "keys", "points", "scaling_raw", "rotation", "normal",
                                    "status", "point_keys", "counts")
    assert hasattr(G.GrowableGaussians, "add_voxel_seeds")
    for m in ("sweep", "loss_points", "state", "grow"):
        assert callable(getattr(G.SweepVoxelMap, m))


def test_the_size_queries():
    L = G.lib()
    for c in (1, 2, 8, 1 << 16, 1 << 26):
        assert L.gsr_voxel_table_bytes(c) == 128 * c
    for c in (0, -8, 3, 48, (1 << 16) + 1, 1 << 27):
        assert L.gsr_voxel_table_bytes(c) == 0, c
    ws = L.gsr_voxel_sweep_workspace
    assert ws(0) == 0 and ws(-1) == 0 and ws((1 << 22) + 1) == 0
    prev = 0
    for n in (1, 255, 256, 257, 100000, 1 << 22):
        assert ws(n) >= max(prev, 5 * n) and ws(n) < 6 * n + 4096
        prev = ws(n)


def test_scalars_are_refused():
    L = G.lib()
    err = L.gsr_last_error
    for n in (-1, (1 << 22) + 1):
        assert _sweep(L, n=n) == -1 and b"bad n" in err(), n
    for m in (0, -3, (1 << 20) + 1):
        assert _sweep(L, min_points=m) == -1 and b"bad min_points" in err(), m
    for name, arg in (("grid", "grid"), ("min_sigma", "min_sigma"), ("scale_factor", "sf")):
        for v in (0.0, -0.2, INF, -INF, math.nan):
            assert _sweep(L, **{arg: v}) == -1 and ("bad " + name).encode() in err(), (name, v)
    for c in (0, -64, 48, 1 << 27):
        assert _sweep(L, capacity=c) == -1 and b"bad capacity" in err(), c
    for v in (-1, 65):
        assert _sweep(L, live=v) == -1 and b"bad live_before" in err(), v
    assert _sweep(L, n=1 << 22, min_points=1 << 20, capacity=1 << 26, live=1 << 26, table=NULL) == -1 and b"null" in err()


def test_pointers_are_refused():
    L = G.lib()
    err = L.gsr_last_error
    for name in NAMES:
        if name not in ("colors", "rgb"):
            assert _sweep(L, **{name: NULL}) == -1 and b"null pointer" in err(), name
    assert _sweep(L, colors=ONE) == -1 and b"null pointer" in err()              # colours without a place for them
    assert _sweep(L, ws=NULL) == -1 and b"null pointer" in err()
    assert _sweep(L, short=1) == -1 and b"workspace too small" in err()
    for name in NAMES:
        if name in ("status",):
            continue
        kw = {name: C.c_void_p(258)}
        if name in ("colors", "rgb"):
            kw.update(colors=kw.get("colors", ONE), rgb=kw.get("rgb", ONE))
        assert _sweep(L, **kw) == -1 and b"misaligned" in err(), name
    for name in ("table", "point_keys", "keys"):
        assert _sweep(L, **{name: C.c_void_p(260)}) == -1 and b"8-byte" in err(), name
    # n == 0 needs the table and the counts only
    assert _sweep(L, n=0, points=NULL, status=NULL, xyz=NULL, table=NULL) == -1 and b"null pointer" in err()
    assert _sweep(L, n=0, counts=NULL) == -1 and b"null pointer" in err()


def test_the_order_of_the_checks():
    L = G.lib()
    err = L.gsr_last_error
    assert _sweep(L, n=-1, min_points=0) == -1 and b"bad n" in err()
    assert _sweep(L, min_points=0, grid=0.0) == -1 and b"bad min_points" in err()
    assert _sweep(L, grid=0.0, min_sigma=0.0) == -1 and b"bad grid" in err()
    assert _sweep(L, min_sigma=0.0, sf=0.0) == -1 and b"bad min_sigma" in err()
    assert _sweep(L, sf=0.0, capacity=3) == -1 and b"bad scale_factor" in err()
    assert _sweep(L, capacity=3, live=-1) == -1 and b"bad capacity" in err()
    assert _sweep(L, live=-1, table=NULL) == -1 and b"bad live_before" in err()
    assert _sweep(L, table=NULL, short=1) == -1 and b"null pointer" in err()
    assert _sweep(L, short=1, xyz=C.c_void_p(258)) == -1 and b"workspace too small" in err()
    assert _sweep(L, xyz=C.c_void_p(258), table=C.c_void_p(260)) == -1 and b"4-byte" in err()


def test_rehash_refusals():
    L = G.lib()
    err = L.gsr_last_error
    a, b = ONE, C.c_void_p(512)
    for cs, cd in ((0, 64), (48, 64), (64, 0), (64, 96), (1 << 27, 1 << 27)):
        assert L.gsr_voxel_rehash(a, cs, b, cd, NULL) == -1 and b"bad capacity" in err(), (cs, cd)
    assert L.gsr_voxel_rehash(a, 128, b, 64, NULL) == -1 and b"smaller" in err()
    assert L.gsr_voxel_rehash(NULL, 64, b, 64, NULL) == -1 and b"null pointer" in err()
    assert L.gsr_voxel_rehash(a, 64, NULL, 64, NULL) == -1 and b"null pointer" in err()
    assert L.gsr_voxel_rehash(C.c_void_p(260), 64, b, 64, NULL) == -1 and b"8-byte" in err()
    assert L.gsr_voxel_rehash(a, 64, a, 64, NULL) == -1 and b"one table" in err()


def test_capi_raises_on_a_refusal():
    with pytest.raises(G.GsrError):
        G._capi.voxel_table(48, "cpu")
    with pytest.raises((G.GsrError, AssertionError)):
        G._capi.voxel_sweep(torch.zeros((4, 3)), None, 0.2, 10, 0.001, 1.0, torch.zeros((64, 16), dtype=torch.int64), 0)
    with pytest.raises(TypeError):
        G.SweepVoxelMap(0.2)                                                      # the policy has no default
