"""CPU tests of the argument validation of gsr_pose_gradient_workspace and gsr_pose_gradient (no device involved:
validation comes first, and nothing is enqueued or written on a refusal)."""
import ctypes as C
import math

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1            # GSR_ERR_INVALID_ARGUMENT
CANARY = 12345.5


def ptr(offset=0):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(4096 + offset)


def _err(L):
    return L.gsr_last_error()


def _call(L, P=1000, W=64, H=48, tanx=0.5, tany=0.4, short=0, **over):
    """-> (return code, the six output floats): the output is host memory with a canary, which a refusal leaves alone
    (nothing is enqueued that could write it, and the host code does not)."""
    out = (C.c_float * 6)(*([CANARY] * 6))
    p = dict(means=ptr(), scales=ptr(), rot=ptr(), cov=NULL, view=ptr(), proj=ptr(), radii=ptr(), g2=ptr(), gc=ptr(),
             gz=NULL, g3=ptr(), out=C.cast(out, C.c_void_p), ws=ptr())
    p.update(over)
    nbytes = max(int(L.gsr_pose_gradient_workspace(P)) - short, 0)
    rc = L.gsr_pose_gradient(P, W, H, p["means"], p["scales"], 1.0, p["rot"], p["cov"], p["view"], p["proj"], tanx, tany,
                             p["radii"], p["g2"], p["gc"], p["gz"], p["g3"], p["out"], p["ws"], nbytes, NULL)
    return rc, list(out)


def _refused(L, what, **kw):
    rc, out = _call(L, **kw)
    assert rc == INVALID, (kw, rc)
    assert what in _err(L), (kw, _err(L))
    assert out == [CANARY] * 6, kw


def test_symbols_and_kernels_are_registered():
    L = G.lib()
    for n in ("gsr_pose_gradient", "gsr_pose_gradient_workspace"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    at = names.index("k_densify_apply") + 1                      # behind adaptive density control
    assert names[at:at + 2] == ["k_pose_partials", "k_pose_finish"]
    assert len(set(names)) == len(names) <= 64                   # the profiler's mask has 64 bits
    assert L.gsr_abi_version() == 2
    assert hasattr(G, "pose_gradient") and hasattr(G, "se3_exp") and hasattr(G.Camera, "retract")


def test_workspace_is_monotone_and_zero_only_for_a_refused_P():
    L = G.lib()
    assert L.gsr_pose_gradient_workspace(-1) == 0 and L.gsr_pose_gradient_workspace(-2 ** 31) == 0
    last = 0
    for P in (0, 1, 255, 256, 257, 4097, 65_536, 65_537, 300_007, 2_000_000, 2 ** 31 - 1):
        need = int(L.gsr_pose_gradient_workspace(P))
        assert need > 0 and need >= last, (P, need)
        assert need <= 48 * ((P + 255) // 256) + 64, (P, need)   # one double[6] per 256 rows + the alignment slack
        last = need
    # a function of P alone: asked twice, the same
    assert L.gsr_pose_gradient_workspace(300_007) == L.gsr_pose_gradient_workspace(300_007)


def test_refusals():
    L = G.lib()
    for P in (-1, -2 ** 31):
        _refused(L, b"bad P", P=P)
    for W, H in ((0, 48), (64, 0), (-3, 48), (64, -1)):
        _refused(L, b"width/height", W=W, H=H)
    for bad in (0.0, -0.5, math.inf, -math.inf, math.nan):
        _refused(L, b"tan_fov", tanx=bad)
        _refused(L, b"tan_fov", tany=bad)
    for name in ("means", "view", "proj", "radii", "g2", "gc", "g3", "ws"):
        _refused(L, b"null", **{name: NULL})
    rc = L.gsr_pose_gradient(1000, 64, 48, ptr(), ptr(), 1.0, ptr(), NULL, ptr(), ptr(), 0.5, 0.4, ptr(), ptr(), ptr(),
                             NULL, ptr(), NULL, ptr(), 1 << 20, NULL)
    assert rc == INVALID and b"null dL_dpose" in _err(L)
    # the covariance inputs: scales without rotations (and the reverse), both with cov3D_precomp, none of the three
    _refused(L, b"either scales+rotations or", rot=NULL)
    _refused(L, b"either scales+rotations or", scales=NULL)
    _refused(L, b"either scales+rotations or", cov=ptr())
    _refused(L, b"either scales+rotations or", scales=NULL, rot=NULL)
    for off in (4, 8, 12):
        _refused(L, b"16-byte aligned", rot=ptr(off))
    for P in (1, 256, 257, 300_007):
        need = int(L.gsr_pose_gradient_workspace(P))
        _refused(L, b"workspace too small", P=P, short=1)
        assert str(need).encode() in _err(L)
    # dL_ddepths is the one nullable gradient input; cov3D_precomp alone is a valid covariance input; neither call gets
    # past the workspace check here
    _refused(L, b"workspace too small", gz=ptr(), short=1)
    _refused(L, b"workspace too small", scales=NULL, rot=NULL, cov=ptr(), short=1)
    # the order: shape, then the camera, then null pointers, then the covariance inputs, then the workspace
    _refused(L, b"bad P", P=-1, W=0, tanx=0.0, means=NULL)
    _refused(L, b"width/height", W=0, tanx=0.0, means=NULL)
    _refused(L, b"tan_fov", tanx=0.0, means=NULL)
    _refused(L, b"null", means=NULL, rot=NULL, short=1)
    _refused(L, b"either scales+rotations or", rot=NULL, short=1)
