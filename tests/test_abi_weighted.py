"""CPU tests of the argument validation of gsr_weighted_loss_workspace and gsr_weighted_loss (no device involved:
validation comes first, and nothing is enqueued or written on a refusal)."""
import ctypes as C

import gs_livm_amd as G

NULL = C.c_void_p(None)
INVALID = -1            # GSR_ERR_INVALID_ARGUMENT
WIN = (C.c_float * 11)(*([1.0 / 11] * 11))


def ptr(offset=0):
    """a non-null address at a byte offset from a 16-byte boundary; never dereferenced: validation fails first"""
    return C.c_void_p(4096 + offset)


def _loss(L, shape=(3, 33, 55), short=0, acc_min=0.5, **over):
    p = dict(img=ptr(), gt=ptr(), w=ptr(), acc=ptr(), e=ptr(), win=WIN, out6=ptr(), gi=ptr(), ge=ptr(), ws=ptr())
    p.update(over)
    nbytes = max(int(L.gsr_weighted_loss_workspace(*shape)) - short, 0)
    return L.gsr_weighted_loss(*shape, p["img"], p["gt"], p["w"], p["acc"], acc_min, p["e"], p["win"], 0.2, p["out6"],
                               p["gi"], p["ge"], p["ws"], nbytes, NULL)


def _refused(L, what, **kw):
    assert _loss(L, **kw) == INVALID, kw
    assert what in L.gsr_last_error(), (kw, L.gsr_last_error())


def test_symbols_are_registered_and_no_kernel_id_is_added():
    L = G.lib()
    for n in ("gsr_weighted_loss", "gsr_weighted_loss_workspace"):
        assert n in G._capi.EXPORTS and hasattr(L, n), n
    names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
    assert len(set(names)) == len(names) <= 64                    # the profiler's mask has 64 bits
    assert not [n for n in names if "weighted" in n]              # timed under the exposure loss's three ids
    assert L.gsr_abi_version() == 2
    for n in ("weighted_photometric_loss", "WeightedPhotometricLoss"):
        assert hasattr(G, n) and n in G.__all__, n


def test_workspace_is_monotone_and_zero_for_a_refused_shape():
    L = G.lib()
    for bad in ((0, 8, 8), (3, 0, 8), (3, 8, 0), (-1, 8, 8), (3, -2 ** 31, 8), (3, 65536, 32768), (1, 2 ** 31 - 1, 1)):
        assert L.gsr_weighted_loss_workspace(*bad) == 0, bad
    last = 0
    for shape in ((1, 1, 1), (1, 1, 2), (1, 32, 54), (1, 33, 54), (1, 33, 55), (3, 33, 55), (3, 480, 640),
                  (3, 1080, 1920), (4, 1080, 1920), (4, 40000, 50000)):
        need = int(L.gsr_weighted_loss_workspace(*shape))
        assert need > 0 and need >= last, (shape, need)
        last = need
        Cn, H, W = shape
        units = Cn * ((H + 31) // 32) * ((W + 53) // 54)
        # the exposure loss's bytes and two more floats per work unit (and the carve's alignment): nothing else
        assert need <= int(L.gsr_exposure_loss_workspace(*shape)) + 8 * units + 256, shape
        assert need >= 12 * Cn * H * W + 32 * units, shape


def test_refusals_and_their_order():
    L = G.lib()
    assert _loss(L, shape=(1, 2 ** 31 - 1, 1)) == INVALID
    for shape in ((0, 33, 55), (3, 0, 55), (3, 33, 0), (-1, 33, 55), (3, 33, -5)):
        _refused(L, b"bad image shape", shape=shape)
    _refused(L, b"image plane too large", shape=(3, 65536, 32768))
    _refused(L, b"image plane too large", shape=(1, 2 ** 31 - 1, 1))
    for name in ("img", "gt", "win", "out6", "ws"):
        _refused(L, b"null pointer", **{name: NULL if name != "win" else None})
    _refused(L, b"without an exposure", e=NULL)                       # dL_dexposure without exposure
    _refused(L, b"without an exposure", e=NULL, gi=NULL)
    _refused(L, b"both or neither", gi=NULL)                          # exposure with only one of the two gradients
    _refused(L, b"both or neither", ge=NULL)
    for bad in (float("nan"), float("inf"), float("-inf")):
        _refused(L, b"acc_min must be finite", acc_min=bad)
    for shape in ((1, 1, 1), (3, 33, 55), (3, 480, 640)):
        _refused(L, b"workspace too small", shape=shape, short=1)
        assert str(int(L.gsr_weighted_loss_workspace(*shape))).encode() in L.gsr_last_error()
    _refused(L, b"workspace too small", gi=NULL, ge=NULL, short=1)   # no gradient: the same workspace is asked for
    _refused(L, b"workspace too small", w=NULL, acc=NULL, e=NULL, ge=NULL, short=1)
    # the order: shape, plane, null pointers, the exposure's gradients, acc_min, the workspace
    _refused(L, b"bad image shape", shape=(0, 65536, 32768), img=NULL, e=NULL)
    _refused(L, b"image plane too large", shape=(3, 65536, 32768), img=NULL, e=NULL)
    _refused(L, b"null pointer", out6=NULL, e=NULL, acc_min=float("nan"), short=1)
    _refused(L, b"without an exposure", e=NULL, acc_min=float("nan"), short=1)
    _refused(L, b"both or neither", ge=NULL, acc_min=float("nan"), short=1)
    _refused(L, b"acc_min must be finite", acc_min=float("nan"), short=1)


def test_absent_operands_are_not_refusals():
    """weights, acc and exposure are optional each; without acc a non-finite acc_min is not looked at.  (Only the
    refusal that follows the accepted checks is observable here: the workspace one byte short.)"""
    L = G.lib()
    for kw in (dict(w=NULL), dict(acc=NULL, acc_min=float("nan")), dict(e=NULL, ge=NULL), dict(e=NULL, ge=NULL, gi=NULL),
               dict(w=NULL, acc=NULL, e=NULL, ge=NULL, gi=NULL, acc_min=float("inf"))):
        _refused(L, b"workspace too small", short=1, **kw)
