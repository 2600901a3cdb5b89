"""GPU tests of the map-growth kernels (csrc/growth.hip) at their edges.

k_init_gaussians against the float64 restatement in tests/growth_ref.py at max(2 e_ref, floor) (floors derived there),
IEEE classes against the float32 restatement, on diagonals over 60 decades, products of exactly 1, subnormal, zero,
negative and overflowing ones; written into views that start at row `lo` of NaN-patterned capacity buffers so that the
output pointers fall at every 4-byte alignment; rows either side keep their bits; xyz is copied bit for bit; rotation,
opacity and f_rest are exact.  k_pack_ply_rows bit for bit against ply.rows_numpy for every M, row counts at the seams
of its 256-thread workgroups, inputs with a bit pattern of their own in every element, guard words behind the rows."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import ply
import growth_ref as R

pytestmark = pytest.mark.gpu
PAT = 0x7FC0DEAD
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def _tails(M):
    return {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (M - 1, 3), "_scaling": (3,), "_rotation": (4,),
            "_opacity": (1,)}


def _check_rows(rows, xyz, covs, rgbs, scale, M, what):
    """rows: {name: [n, ...] device tensors} as written by the kernel."""
    n = xyz.shape[0]
    assert torch.equal(R.bits(rows["_xyz"].cpu()), R.bits(xyz)), "xyz is not a bit copy"
    rot = torch.zeros((n, 4))
    rot[:, 0] = 1.0
    assert torch.equal(R.bits(rows["_rotation"].cpu()), R.bits(rot))
    assert not bool(R.bits(rows["_opacity"].cpu()).any())
    assert rows["_features_rest"].shape == (n, M - 1, 3) and not bool(R.bits(rows["_features_rest"].cpu()).any())
    res = R.judge(rows["_scaling"], rows["_features_dc"], covs, rgbs, scale)
    print(json.dumps(dict(what=what, n=n, M=M, scale=scale,
                          figures={k: ["%.3g" % x for x in v] for k, v in res.items()})))
    for k, v in res.items():
        assert v[2] <= 1.0, "%s %s: err %.3g, e_ref %.3g: %.3g of the bar" % (what, k, v[0], v[1], v[2])


CASES = [(n, R.MS[i % 6], R.LOS[i % 5], R.SCALES[i % 3]) for i, n in enumerate(R.NS * 3)] + \
        [(257, M, lo, 4.0) for M, lo in ((2, 1), (3, 3), (9, 2), (16, 257), (1, 1), (4, 0))]


@pytest.mark.parametrize("n,M,lo,scale", CASES)
def test_init_kernel_against_float64_in_guarded_capacity_buffers(n, M, lo, scale, gpu_device):
    xyz, covs, rgbs = R.cloud(n, 1, scale)
    cap = lo + n + 5
    buf = {k: torch.full((cap,) + t, PAT, dtype=torch.int32, device=gpu_device).view(torch.float32)
           for k, t in _tails(M).items()}
    view = {k: b[lo:lo + n] for k, b in buf.items()}
    if M > 1:   # the four-byte alignments the row offset produces
        assert view["_features_rest"].data_ptr() % 16 == (lo * 3 * (M - 1) * 4) % 16
    G._capi.init_gaussians(xyz.to(gpu_device), covs.to(gpu_device), rgbs.to(gpu_device), scale, *[view[k] for k in NAMES])
    torch.cuda.synchronize()
    for k, b in buf.items():
        i = b.view(torch.int32)
        assert bool((i[:lo] == PAT).all()) and bool((i[lo + n:] == PAT).all()), "%s: a row outside [lo, lo + n) was written" % k
    _check_rows(view, xyz, covs, rgbs, scale, M, "init lo=%d" % lo)


def test_add_new_pointcloud_across_a_capacity_doubling(gpu_device):
    M = 3
    m = G.GrowableGaussians(300, M, gpu_device)
    clouds = [R.cloud(n, 2 + i, s) for i, (n, s) in enumerate(((257, 1.7), (255, 4.0), (4097, 0.5)))]
    at, spans = 0, []
    for (xyz, covs, rgbs), s in zip(clouds, (1.7, 4.0, 0.5)):
        old = {k: R.bits(getattr(m, k).detach()).clone() for k in NAMES}
        cap = m.capacity
        lo, hi = m.add_new_pointcloud(xyz.to(gpu_device), covs.to(gpu_device), rgbs.to(gpu_device), scale_factor=s)
        assert (lo, hi) == (at, at + xyz.shape[0]) and m.P == hi
        spans.append((cap, m.capacity))
        for k in NAMES:   # the old rows keep their bits, through the reallocation too
            assert torch.equal(R.bits(getattr(m, k).detach())[:lo], old[k]), k
        _check_rows({k: getattr(m, k).detach()[lo:hi] for k in NAMES}, xyz, covs, rgbs, s, M, "add_new_pointcloud")
        at = hi
    assert spans[0][0] == spans[0][1] and spans[1][1] > spans[1][0] and spans[2][1] > spans[2][0]   # fits, doubles, doubles
    # rows beyond P are still the zeros the buffers were created with
    for k in NAMES:
        assert not bool(R.bits(m._buf[k][m.P:]).any()), k


def _patterned(P, M, dev):
    """Six leaves whose every element has a bit pattern of its own: (leaf index << 28) | running element number, plus
    -0.0, subnormals and NaNs with payloads in the first rows."""
    out, host = [], {}
    for j, (k, t) in enumerate(_tails(M).items()):
        n = P * int(np.prod(t))
        a = (np.arange(n, dtype=np.uint32) + np.uint32(1)) | np.uint32((j + 1) << 28)
        sp = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F800001], dtype=np.uint32)
        a[:min(n, 6)] = sp[:min(n, 6)] if j % 2 == 0 else a[:min(n, 6)]
        host[k] = a.view(np.float32).reshape((P,) + t)
        out.append(torch.from_numpy(host[k].copy()).to(dev))
    return out, host


def _seam_rows(M):
    """Row counts P with P * (14 + 3 M) just below, on and just above a multiple of the 256 threads of a workgroup: the
    residues -g, 0, +g mod 256, g = gcd(14 + 3 M, 256) being the nearest that a whole number of rows can reach (g = 1 for
    odd M: 255 / 256 / 257; g = 2, 4, 8 or 32 for even M)."""
    rf = 14 + 3 * M
    g = math.gcd(rf, 256)
    out = []
    for r in (256 - g, 0, g):
        out.append(next(P for P in range(1, 257) if (P * rf) % 256 == r % 256))
    return out


PACK = sorted({(M, P) for M in range(1, 17) for P in _seam_rows(M) + [1]})
PACK += [(M, 3001) for M in (1, 2, 3, 4, 16)]


@pytest.mark.parametrize("M,P", PACK)
def test_pack_ply_rows_bit_for_bit_with_guards(M, P, gpu_device):
    (xyz, fdc, frest, scaling, rotation, opacity), host = _patterned(P, M, gpu_device)
    rf = 14 + 3 * M
    total = P * rf
    for lead in (4, 5):   # rows at 0 and 4 bytes past a 16-byte boundary
        buf = torch.full((total + 16,), PAT, dtype=torch.int32, device=gpu_device)
        rows = buf.view(torch.float32)[lead:lead + total]
        L = G._capi.lib()
        p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
        code = L.gsr_pack_ply_rows(P, M, p(xyz), p(fdc), p(frest), p(opacity), p(scaling), p(rotation), p(rows),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert code == 0, L.gsr_last_error()
        assert bool((buf[:lead] == PAT).all()) and bool((buf[lead + total:] == PAT).all()), "guard overwritten"
        want = ply.rows_numpy(host["_xyz"], host["_features_dc"], host["_features_rest"], host["_opacity"],
                              host["_scaling"], host["_rotation"])
        got = rows.cpu().numpy().reshape(P, rf)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    via = G._capi.pack_ply_rows(xyz, fdc, frest, opacity, scaling, rotation).cpu().numpy()
    assert np.array_equal(via.view(np.uint32), want.view(np.uint32))
