"""CPU tests of the restatement the point-to-plane loss is held to (tests/plane_ref.py): its gradients, the pairing of
the columns of R(q) with the scales (proved against the oracle's 3-D covariance, not taken from a text), the round trip
of a voxel seed, and the share of fragile points of every GPU case."""
import functools
import math

import numpy as np
import pytest
import torch

import plane_ref as PR
from gs_livm_amd import synthetic as S
from oracle import oracle as O

EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _inputs(m, n):
    return PR.case_inputs(m, n)


@pytest.mark.parametrize("params", [PR.PARAMS[0], (0.02, float("inf"), 0.3), (0.02, 0.08, 0.3)],
                         ids=["abs", "huber", "huber-gated"])
def test_gradcheck_of_the_float64_restatement(params):
    c = _inputs(7, 16)
    huber, max_dist, lambda_flat = params
    idx = c["sel"].long()
    rows = torch.arange(16, dtype=torch.int32)
    x, s, q = (c[k].double().index_select(0, idx).clone().requires_grad_(True) for k in ("xyz", "scaling", "rotation"))
    a = PR.analyse(c["points"], rows, x.detach(), s.detach(), q.detach(), params)
    assert not bool(a["fragile"].any())          # (finite differences must not cross a comparison)
    assert bool(a["gate"].any())
    if huber > 0 and max_dist == float("inf"):
        assert bool(a["knee"].any()) and bool((~a["knee"]).any())
    if max_dist < float("inf"):
        assert not bool(a["gate"].all())
    fn = lambda x_, s_, q_: PR.plane_loss_ref(c["points"].double(), rows, x_, s_, q_, PR.LAM, huber, max_dist,  # noqa: E731
                                              lambda_flat)
    assert torch.autograd.gradcheck(fn, (x, s, q), eps=1e-7, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("params", PR.PARAMS)
@pytest.mark.parametrize("m,n", [(7, 16), (65, 272)])
def test_the_written_out_gradients_equal_autograd(m, n, params):
    c = _inputs(m, n)
    args = [c[k].double() if k != "sel" else c[k] for k in ("points", "sel", "xyz", "scaling", "rotation")]
    a = PR.reference(*args, params, torch.float64)
    b = PR.plane_loss_closed(*args, params)
    for k in ("out4", "gx", "gs", "gr"):
        torch.testing.assert_close(b[k], a[k], rtol=1e-12, atol=1e-15)
    assert bool(a["gr"].index_select(0, c["sel"].long())[:, 0].any())        # the w component is alive
    # every mutant is a different function (which check of the GPU test refuses it is that file's business); seven
    # points may all lie on one side of their planes, so the larger case decides
    for mutant in PR.MUTANTS if m >= 65 else ():
        if mutant == "gate_on_d2" and params[1] == float("inf") or mutant == "huber_slope_halved" and params[0] == 0:
            continue
        w = PR.plane_loss_closed(*args, params, mutant=mutant)
        assert any(not torch.allclose(w[k], a[k], rtol=1e-6, atol=0) for k in ("out4", "gx", "gr")), mutant


def _oracle_cov(scales, rotations):
    """The oracle's 3-D covariance [P,3,3] (float32 arithmetic) of Gaussians placed in front of a camera."""
    P = scales.shape[0]
    tanx, tany, W, H = 0.5, 0.375, 64, 48
    view = np.eye(4, dtype=np.float32)
    proj = S.projection_matrix(S.ZNEAR, S.ZFAR, 2 * math.atan(tanx), 2 * math.atan(tany)).T.copy()
    means = np.zeros((P, 3), np.float32)
    means[:, 2] = 3.0
    sc = dict(W=W, H=H, tanfovx=tanx, tanfovy=tany, viewmatrix=view, projmatrix=(view @ proj).astype(np.float32),
              campos=np.zeros(3, np.float32), bg=np.ones(3, np.float32), means3D=means, scales=scales,
              rotations=rotations, opacities=np.full((P, 1), 0.5, np.float32), shs=np.zeros((P, 1, 3), np.float32),
              sh_degree=0, colors_precomp=None, cov3D_precomp=None)
    c6 = O.forward(sc, keep_handle=False).cov3D.astype(np.float64)
    cov = np.empty((P, 3, 3))
    for (r, c), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        cov[:, r, c] = cov[:, c, r] = c6[:, k]
    return cov


def test_column_k_of_R_is_the_axis_of_scale_k():
    """Sigma = sum_k s_k^2 a_k a_k^T with a_k = COLUMN k of the restatement's R(q) is the oracle's 3-D covariance within
    the roundings of its float32 arithmetic, and the eigenvector of the smallest eigenvalue of that covariance is +-n.
    The bound: an entry of R is a sum of monomials of q whose absolute values add up to at most N = 1 + 2|q|^2, four
    roundings; one more for the product with s; an entry of M^T M is three products and two additions; so an entry
    of Sigma is off by at most (2 (4 + 1) + 3) eps32 sum_k s_k^2 N^2."""
    rng = np.random.default_rng(5)
    P = 64
    scales = rng.uniform(0.02, 0.1, (P, 3))
    thin = rng.integers(0, 3, P)
    scales[np.arange(P), thin] = scales.min(1) * rng.uniform(0.2, 0.5, P)
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1
    scales, q = scales.astype(np.float32), q.astype(np.float32)
    cov = _oracle_cov(scales, q)
    R = PR.rotation_matrix(torch.from_numpy(q).double()).numpy()
    s2 = scales.astype(np.float64) ** 2
    ours = np.einsum("pik,pk,pjk->pij", R, s2, R)              # columns paired with scales
    swapped = np.einsum("pki,pk,pkj->pij", R, s2, R)           # rows paired with scales: the transposed convention
    N = 1 + 2 * (q.astype(np.float64) ** 2).sum(1)
    bound = 13 * EPS32 * s2.sum(1) * N ** 2
    assert bool((np.abs(ours - cov).max((1, 2)) <= bound).all())
    assert bool((np.abs(swapped - cov).max((1, 2)) > 100 * bound).all())    # (the check tells the two apart)
    # the thin axis: k* = argmin of the scales, n = that column; Davis-Kahan: sin(angle) <= 2 |dSigma|_F / gap
    ks = torch.from_numpy(scales).argmin(1).numpy()
    assert np.array_equal(ks, thin)
    n = R[np.arange(P), :, ks]
    lam, vec = np.linalg.eigh(cov)
    u = vec[:, :, 0]
    sin = np.linalg.norm(np.cross(n, u), axis=1)
    srt = np.sort(s2, 1)
    assert bool((sin <= 2 * 3 * bound / (srt[:, 1] - srt[:, 0])).all()) and float(sin.max()) < 0.05
    assert bool((np.abs((n * u).sum(1)) > 0.99).all())


def test_a_voxel_seed_has_its_normal_in_column_2():
    """A surfel built as the sweep voxel map builds its seeds (csrc/voxel.hip): eigen-decomposition of the voxel's
    covariance, eigenvalues DESCENDING, right-handed axes in the columns of V, the quaternion of V with w >= 0,
    scales sqrt(lambda).  The point-to-plane term then picks k* = 2 and its n is parallel to the seed's normal."""
    rng = np.random.default_rng(12)
    for _ in range(32):
        basis = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        pts = (rng.standard_normal((40, 3)) * np.array([0.06, 0.03, 0.004])) @ basis.T
        lam, V = np.linalg.eigh(np.cov(pts.T))
        lam, V = lam[::-1].copy(), V[:, ::-1].copy()
        if np.linalg.det(V) < 0:
            V[:, 2] = -V[:, 2]
        tr = V[0, 0] + V[1, 1] + V[2, 2]
        if tr > 0:
            s = 2 * math.sqrt(tr + 1)
            q = [0.25 * s, (V[2, 1] - V[1, 2]) / s, (V[0, 2] - V[2, 0]) / s, (V[1, 0] - V[0, 1]) / s]
        elif V[0, 0] > V[1, 1] and V[0, 0] > V[2, 2]:
            s = 2 * math.sqrt(1 + V[0, 0] - V[1, 1] - V[2, 2])
            q = [(V[2, 1] - V[1, 2]) / s, 0.25 * s, (V[0, 1] + V[1, 0]) / s, (V[0, 2] + V[2, 0]) / s]
        elif V[1, 1] > V[2, 2]:
            s = 2 * math.sqrt(1 + V[1, 1] - V[0, 0] - V[2, 2])
            q = [(V[0, 2] - V[2, 0]) / s, (V[0, 1] + V[1, 0]) / s, 0.25 * s, (V[1, 2] + V[2, 1]) / s]
        else:
            s = 2 * math.sqrt(1 + V[2, 2] - V[0, 0] - V[1, 1])
            q = [(V[1, 0] - V[0, 1]) / s, (V[0, 2] + V[2, 0]) / s, (V[1, 2] + V[2, 1]) / s, 0.25 * s]
        q = np.array(q) / np.linalg.norm(q)
        q = (q if q[0] >= 0 else -q).astype(np.float32)
        scales = torch.from_numpy(np.sqrt(lam).astype(np.float32))
        normal = V[:, 2].astype(np.float32)
        assert int(scales.argmin()) == 2
        n = PR.rotation_matrix(torch.from_numpy(q))[:, 2].numpy()
        assert abs(float(n @ normal)) > 1 - 16 * EPS32 and np.linalg.norm(np.cross(n, normal)) < 1e-3
        # and a point of the voxel lies on the plane within the thin scale, not within the wide ones
        c = dict(points=torch.from_numpy(pts.astype(np.float32)), sel=torch.zeros(1, dtype=torch.int32),
                 xyz=torch.from_numpy(pts.mean(0, keepdims=True).astype(np.float32)), scaling=scales[None],
                 rotation=torch.from_numpy(q)[None])
        a = PR.analyse(c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"], PR.PARAMS[0])
        assert float(a["e"].abs().mean()) < 2 * float(scales[2]) < float(a["d"].mean())


@pytest.mark.parametrize("params", PR.PARAMS)
@pytest.mark.parametrize("m,n", list(PR.CASES))
def test_fragile_share_of_every_gpu_case(m, n, params):
    """At most 1 % of a case's points may be removed as fragile (a cap, not a tolerance); float64 only."""
    c = _inputs(m, n)
    a = PR.analyse(c["points"], c["sel"], c["xyz"], c["scaling"], c["rotation"], params)
    removed = int(a["fragile"].sum())
    print(dict(m=m, n=n, params=params, removed=removed, gated_in=float(a["gate"].double().mean()),
               in_knee=float((a["knee"] & a["gate"]).double().mean()), median_abs_e=float(a["e"].abs().median()),
               median_d=float(a["d"].median())))
    assert removed <= 0.01 * m
    if m >= 65:      # both sides of the gate and of the knee are populated
        if params[1] < float("inf"):
            assert 0.1 < float(a["gate"].double().mean()) < 0.9
        if params[0] > 0:
            g = a["gate"]
            assert bool((a["knee"] & g).any()) and bool((~a["knee"] & g).any())
