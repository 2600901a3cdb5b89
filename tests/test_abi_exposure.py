"""CPU tests of the argument validation of gsr_exposure_loss_workspace, gsr_exposure_loss and gsr_apply_exposure (no
device involved: validation comes first, and nothing is enqueued or written on a refusal)."""
import ctypes as C

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1            # GSR_ERR_INVALID_ARGUMENT
WIN = (C.c_float * 11)(*([1.0 / 11] * 11))


def ptr(offset=0):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(4096 + offset)


def _loss(L, shape=(3, 33, 55), short=0, **over):
    p = dict(img=ptr(), gt=ptr(), e=ptr(), win=WIN, out3=ptr(), gi=ptr(), ge=ptr(), ws=ptr())
    p.update(over)
    nbytes = max(int(L.gsr_exposure_loss_workspace(*shape)) - short, 0)
    return L.gsr_exposure_loss(*shape, p["img"], p["gt"], p["e"], p["win"], 0.2, p["out3"], p["gi"], p["ge"], p["ws"],
                               nbytes, NULL)


def _refused(L, what, **kw):
    assert _loss(L, **kw) == INVALID, kw
    assert what in L.gsr_last_error(), (kw, L.gsr_last_error())


def test_symbols_and_kernels_are_registered():
    L = G.lib()
    for n in ("gsr_exposure_loss", "gsr_exposure_loss_workspace", "gsr_apply_exposure"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    at = names.index("k_pose_finish") + 1                         # directly behind the pose gradient
    assert names[at:at + 4] == ["k_exposure_loss_forward", "k_exposure_loss_backward", "k_exposure_loss_finish",
                                "k_apply_exposure"]
    assert names[at + 4] == "k_metrics_forward"
    assert len(set(names)) == len(names) <= 64                    # the profiler's mask has 64 bits
    assert L.gsr_abi_version() == 2
    for n in ("exposure_photometric_loss", "apply_exposure", "identity_exposure", "ExposureLoss"):
        assert hasattr(G, n) and n in G.__all__, n


def test_workspace_is_monotone_and_zero_for_a_refused_shape():
    L = G.lib()
    for bad in ((0, 8, 8), (3, 0, 8), (3, 8, 0), (-1, 8, 8), (3, -2 ** 31, 8), (3, 65536, 32768), (1, 2 ** 31 - 1, 1)):
        assert L.gsr_exposure_loss_workspace(*bad) == 0, bad
    last = 0
    for shape in ((1, 1, 1), (1, 1, 2), (1, 32, 54), (1, 33, 54), (1, 33, 55), (3, 33, 55), (3, 480, 640),
                  (3, 1080, 1920), (4, 1080, 1920), (4, 40000, 50000)):
        need = int(L.gsr_exposure_loss_workspace(*shape))
        assert need > 0 and need >= last, (shape, need)
        last = need
        Cn, H, W = shape
        units = Cn * ((H + 31) // 32) * ((W + 53) // 54)
        # the plain loss's bytes, one float64 pair per work unit, the slack that aligns them: nothing else
        assert need <= int(L.gsr_photometric_loss_workspace(*shape)) + 16 * units + 16, shape
        assert need >= 12 * Cn * H * W + 24 * units, shape
    assert L.gsr_exposure_loss_workspace(3, 480, 640) == L.gsr_exposure_loss_workspace(3, 480, 640)


def test_loss_refusals_and_their_order():
    L = G.lib()
    for shape in ((0, 33, 55), (3, 0, 55), (3, 33, 0), (-1, 33, 55), (3, 33, -5)):
        _refused(L, b"bad image shape", shape=shape)
    _refused(L, b"image plane too large", shape=(3, 65536, 32768))
    _refused(L, b"image plane too large", shape=(1, 2 ** 31 - 1, 1))
    for name in ("img", "gt", "e", "win", "out3", "ws"):
        _refused(L, b"null pointer", **{name: NULL if name != "win" else None})
    _refused(L, b"both or neither", gi=NULL)
    _refused(L, b"both or neither", ge=NULL)
    for shape in ((1, 1, 1), (3, 33, 55), (3, 480, 640)):
        _refused(L, b"workspace too small", shape=shape, short=1)
        assert str(int(L.gsr_exposure_loss_workspace(*shape))).encode() in L.gsr_last_error()
    _refused(L, b"workspace too small", gi=NULL, ge=NULL, short=1)   # no gradient: the same workspace is asked for
    # the order: shape, plane, null pointers, the gradient pair, the workspace
    _refused(L, b"bad image shape", shape=(0, 65536, 32768), img=NULL, gi=NULL)
    _refused(L, b"image plane too large", shape=(3, 65536, 32768), img=NULL, gi=NULL)
    _refused(L, b"null pointer", e=NULL, gi=NULL, short=1)
    _refused(L, b"both or neither", ge=NULL, short=1)


def test_apply_refusals_and_their_order():
    L = G.lib()
    call = lambda shape=(3, 33, 55), img=ptr(), e=ptr(), out=ptr(): L.gsr_apply_exposure(*shape, img, e, out, NULL)  # noqa: E731

    def refused(what, **kw):
        assert call(**kw) == INVALID, kw
        assert what in L.gsr_last_error(), (kw, L.gsr_last_error())

    for shape in ((0, 33, 55), (3, 0, 55), (3, 33, 0), (3, -1, 55)):
        refused(b"bad image shape", shape=shape)
    refused(b"image plane too large", shape=(3, 65536, 32768))
    for name in ("img", "e", "out"):
        refused(b"null pointer", **{name: NULL})
    for name in ("img", "e", "out"):
        for off in (1, 2, 3):
            refused(b"4-byte alignment", **{name: ptr(off)})
    refused(b"bad image shape", shape=(0, 65536, 32768), img=NULL, out=ptr(1))
    refused(b"image plane too large", shape=(3, 65536, 32768), img=NULL, out=ptr(1))
    refused(b"null pointer", img=NULL, out=ptr(1))
