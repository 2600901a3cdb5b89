"""CPU tests of the argument validation of the normal-map entry points (gsr_blend_attributes, gsr_surfel_normals,
gsr_normal_consistency_workspace, gsr_normal_consistency_loss): no device involved -- validation comes first, and nothing
is enqueued or written on a refusal -- and of what the feature registers (symbols, no new profiler id, Python names)."""
import ctypes as C
import os

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1                  # GSR_ERR_INVALID_ARGUMENT
INF, NAN = float("inf"), float("nan")


def ptr(offset=0, base=1 << 20):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(base + offset)


def _err(L):
    return L.gsr_last_error()


def _blend(L, P=1000, R=5000, W=640, H=480, channels=3, attributes=ptr(0, 5 << 20), geom=ptr(), binning=ptr(0, 2 << 20),
           image=ptr(0, 3 << 20), out=ptr(0, 4 << 20)):
    return L.gsr_blend_attributes(P, R, W, H, channels, attributes, geom, binning, image, out, NULL)


def _normals(L, P=1000, xyz=ptr(), scaling=ptr(0, 2 << 20), rotation=ptr(0, 3 << 20), T=(C.c_float * 12)(), out=ptr(0, 4 << 20)):
    return L.gsr_surfel_normals(P, xyz, scaling, rotation, T, out, NULL)


def _loss(L, H=480, W=640, depth=ptr(), acc=ptr(0, 2 << 20), normals=ptr(0, 3 << 20), fx=500.0, fy=500.0, cx=319.5,
          cy=239.5, acc_min=0.5, normal_min=0.1, jump_rel=INF, lam=1.0, out3=ptr(0, 4 << 20), gd=ptr(0, 5 << 20),
          ga=ptr(0, 6 << 20), ws=ptr(0, 7 << 20), ws_bytes=1 << 40):
    return L.gsr_normal_consistency_loss(H, W, depth, acc, normals, fx, fy, cx, cy, acc_min, normal_min, jump_rel, lam,
                                         out3, gd, ga, ws, ws_bytes, NULL)


def test_symbols_python_names_and_no_new_kernel_id():
    L = G.lib()
    for n in ("gsr_blend_attributes", "gsr_surfel_normals", "gsr_normal_consistency_workspace",
              "gsr_normal_consistency_loss"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names_64.txt")
    with open(golden) as f:
        assert names == f.read().split()        # the profiler word is full: no id was added, none renamed
    assert L.gsr_kernel_count() == 64 and not [k for k in names if "normal" in k or "attribute" in k]
    assert L.gsr_abi_version() == 2
    for n in ("blend_attributes", "render_attributes", "surfel_normals", "render_normals", "NormalConsistencyLoss",
              "normal_consistency_loss"):
        assert n in G.__all__ and hasattr(G, n), n
    for n in ("blend_attributes", "surfel_normals", "normal_consistency_loss"):
        assert hasattr(G._capi, n), n


def test_lambda_and_normal_min_have_no_default():
    import inspect
    p = inspect.signature(G.normal_consistency_loss).parameters
    assert p["lambda_"].default is inspect.Parameter.empty and p["normal_min"].default is inspect.Parameter.empty
    assert p["acc_min"].default == 0.5 and p["jump_rel"].default == INF


def test_workspace_query():
    L = G.lib()
    for H, W in ((0, 5), (5, 0), (-1, 5), (65536, 32768)):
        assert L.gsr_normal_consistency_workspace(H, W) == 0, (H, W)
    # f64 + int partials per 256 pixels, the scale, six parked floats per pixel, carved at 256-byte steps
    small, big = L.gsr_normal_consistency_workspace(3, 3), L.gsr_normal_consistency_workspace(1080, 1920)
    assert 0 < small < 4096
    assert 24 * 1080 * 1920 < big < 24 * 1080 * 1920 + 12 * (1080 * 1920 // 256 + 1) + 4096


def test_blend_refusals_and_their_order():
    L = G.lib()
    for ch in (0, 5, -1, 2 ** 31 - 1):
        assert _blend(L, channels=ch) == INVALID and b"bad channels" in _err(L), ch
    for kw in (dict(P=-1), dict(R=-1), dict(W=0), dict(W=-5), dict(H=0), dict(H=-2 ** 31)):
        assert _blend(L, **kw) == INVALID and b"bad P/R/width/height" in _err(L), kw
    for W, H in ((65536, 32768), (2 ** 31 - 1, 2), (46341, 46341)):      # W * H >= 2^31
        assert _blend(L, W=W, H=H) == INVALID and b"image plane too large" in _err(L), (W, H)
    assert _blend(L, out=NULL) == INVALID and b"null pointer" in _err(L)
    assert _blend(L, attributes=NULL) == INVALID and b"null pointer" in _err(L)
    for name in ("geom", "binning", "image"):
        assert _blend(L, **{name: NULL}) == INVALID and b"null state blob" in _err(L), name
    for off in (1, 2, 3, 5, 7):
        assert _blend(L, out=ptr(off, 4 << 20)) == INVALID and b"4-byte" in _err(L), off
        assert _blend(L, attributes=ptr(off, 5 << 20)) == INVALID and b"4-byte" in _err(L), off
    # the order: channels, counts, the plane, null pointers (out and attributes, then the blobs), alignment
    assert _blend(L, channels=0, P=-1, W=65536, H=32768, out=NULL) == INVALID and b"bad channels" in _err(L)
    assert _blend(L, P=-1, W=65536, H=32768, out=NULL) == INVALID and b"bad P/R" in _err(L)
    assert _blend(L, W=65536, H=32768, out=NULL) == INVALID and b"plane too large" in _err(L)
    assert _blend(L, out=NULL, geom=NULL, attributes=ptr(2)) == INVALID and b"null pointer" in _err(L)
    assert _blend(L, out=ptr(2), geom=NULL) == INVALID and b"null state blob" in _err(L)
    # P == 0 or R == 0: the blobs and the attributes are not looked at -- but out still is, and a bad shape comes first
    for kw in (dict(P=0), dict(R=0)):
        assert _blend(L, out=NULL, geom=NULL, attributes=NULL, **kw) == INVALID and b"null pointer" in _err(L)
        assert _blend(L, out=ptr(2), geom=NULL, binning=NULL, image=NULL, attributes=ptr(1), **kw) == INVALID
        assert b"4-byte" in _err(L)
        assert _blend(L, channels=9, **kw) == INVALID and b"bad channels" in _err(L)


def test_normals_refusals_and_their_order():
    L = G.lib()
    assert _normals(L, P=-1) == INVALID and b"bad P" in _err(L)
    for name in ("xyz", "scaling", "rotation", "out"):
        assert _normals(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    assert _normals(L, T=None) == INVALID and b"null pointer" in _err(L)
    for name in ("xyz", "scaling", "rotation", "out"):
        for off in (1, 2, 3):
            assert _normals(L, **{name: ptr(off, 9 << 20)}) == INVALID and b"4-byte" in _err(L), (name, off)
    assert _normals(L, P=-1, xyz=NULL, out=ptr(1)) == INVALID and b"bad P" in _err(L)
    assert _normals(L, xyz=NULL, out=ptr(1)) == INVALID and b"null pointer" in _err(L)
    # an empty model is legal whatever the pointers: nothing to write, nothing enqueued
    assert _normals(L, P=0, xyz=NULL, scaling=NULL, rotation=NULL, T=None, out=NULL) == 0 and _err(L) == b""


def test_loss_refusals_and_their_order():
    L = G.lib()
    for kw in (dict(H=0), dict(W=0), dict(H=-3)):
        assert _loss(L, **kw) == INVALID and b"bad image shape" in _err(L), kw
    assert _loss(L, W=65536, H=32768) == INVALID and b"image plane too large" in _err(L)
    for name in ("acc_min", "normal_min", "lam"):
        for v in (-1e-9, NAN, -INF):
            text = b"bad lambda" if name == "lam" else b"bad " + name.encode()
            assert _loss(L, **{name: v}) == INVALID and text in _err(L), (name, v)
    for v in (-1e-9, NAN, -INF):
        assert _loss(L, jump_rel=v) == INVALID and b"bad jump_rel" in _err(L), v
    for name in ("fx", "fy"):
        for v in (0.0, -1.0, NAN, INF, -INF):
            assert _loss(L, **{name: v}) == INVALID and b"bad fx / fy" in _err(L), (name, v)
    for name in ("depth", "acc", "normals", "out3", "ws"):
        assert _loss(L, **{name: NULL}) == INVALID and b"null pointer" in _err(L), name
    for name in ("depth", "acc", "normals", "out3", "gd", "ga"):
        for off in (1, 2, 3):
            assert _loss(L, **{name: ptr(off, 9 << 20)}) == INVALID and b"4-byte" in _err(L), (name, off)
    for off in (1, 2, 4, 12):
        assert _loss(L, ws=ptr(off, 7 << 20)) == INVALID and b"8-byte" in _err(L), off
    assert _loss(L, ws_bytes=L.gsr_normal_consistency_workspace(480, 640) - 1) == INVALID and b"workspace too small" in _err(L)
    # the order: shape, plane, acc_min, normal_min, lambda, jump_rel, fx / fy, null pointers, float alignment, workspace
    # alignment, workspace size
    bad = dict(acc_min=-1.0, normal_min=-1.0, lam=-1.0, jump_rel=-1.0, fx=0.0, depth=NULL, acc=ptr(2), ws=ptr(4), ws_bytes=0)
    steps = [(dict(H=0, W=65536), b"bad image shape"), (dict(H=32768, W=65536), b"plane too large"), ({}, b"bad acc_min"),
             (dict(acc_min=0.5), b"bad normal_min"), (dict(normal_min=0.0), b"bad lambda"), (dict(lam=0.0), b"bad jump_rel"),
             (dict(jump_rel=0.0), b"bad fx / fy"), (dict(fx=1.0), b"null pointer"), (dict(depth=ptr()), b"4-byte"),
             (dict(acc=ptr(0, 2 << 20)), b"8-byte"), (dict(ws=ptr(0, 7 << 20)), b"workspace too small")]
    for fix, text in steps:
        if "H" not in fix:
            bad.update(fix)
        assert _loss(L, **dict(bad, **fix)) == INVALID and text in _err(L), (fix, text, _err(L))
    # images without an interior are shapes like any other here: legal, and refused for the same reasons
    assert _loss(L, H=1, W=7, depth=NULL) == INVALID and b"null pointer" in _err(L)
    # zero thresholds and an infinite jump gate are legal values (the next check is reached)
    assert _loss(L, acc_min=0.0, normal_min=0.0, lam=0.0, jump_rel=INF, depth=NULL) == INVALID and b"null pointer" in _err(L)
