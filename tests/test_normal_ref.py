"""CPU tests of the references of the surfel normals and of the depth-normal consistency loss (tests/normal_ref.py):
before the HIP kernels are held to them, they are held to closed forms, to gradcheck and to the recorded yardsticks."""
import math

import numpy as np
import pytest
import torch

import normal_ref as NR


# ---- normals -------------------------------------------------------------------------------------------------------------
def test_normal_rows_cover_ties_and_both_sides_of_the_flip():
    xyz, s, q, T = NR.normal_rows()
    n, fragile = NR.surfel_normals(xyz, s, q, T)
    print("fragile share %.2e" % fragile.mean())
    assert fragile.mean() <= NR.MAX_FRAGILE_SHARE
    # the facing normal: n . p_c <= 0 on every row, and both signs of the un-flipped axis occur
    Tm = T.astype(np.float64)
    p_c = xyz.astype(np.float64) @ Tm[:, :3].T + Tm[:, 3]
    assert ((n * p_c).sum(1) <= 0).all()
    k = np.argmin(s, 1)
    raw = NR._columns(q, np.float64)[np.arange(len(k)), k] @ Tm[:, :3].T
    flipped = (raw * n).sum(1) < 0
    assert 0.2 < flipped.mean() < 0.8
    # exact ties: the lowest index wins
    assert (k[0:10] == 0).all() and (k[10:20] == 1).all() and (k[20:30] == 0).all() and (k[30:40] == 0).all()
    assert (s[0:10, 0] == s[0:10, 1]).all() and (s[10:20, 1] == s[10:20, 2]).all() and (s[30:40, 0] == s[30:40, 2]).all()


def test_identity_quaternion_gives_the_world_axis_of_the_thin_scale():
    xyz = np.array([[0, 0, 3.0]] * 3, np.float32)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (3, 1))
    s = np.array([[0.01, 0.2, 0.2], [0.2, 0.01, 0.2], [0.2, 0.2, 0.01]], np.float32)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    n, fragile = NR.surfel_normals(xyz, s, q, T)
    # x and y axes are perpendicular to the viewing ray (n . p = 0: not flipped, and fragile); z faces away and is flipped
    assert np.array_equal(n, np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]]))
    assert fragile.tolist() == [True, True, False]


def test_normals_yardstick_stays_within_the_recorded_ratio():
    xyz, s, q, T = NR.normal_rows()
    n64, fragile = NR.surfel_normals(xyz, s, q, T)
    n32, _ = NR.surfel_normals(xyz, s, q, T, np.float32)
    d = np.abs(n32.astype(np.float64) - n64).max(1) / np.linalg.norm(n64, axis=1)
    worst = float(d[~fragile].max())
    print("float32 normals worst |d| / |n|: %.3e" % worst)
    assert 0.5 * NR.YARD_NORMALS <= worst <= NR.YARD_NORMALS


# ---- the loss: closed forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_deg", [0.0, 10.0, 75.0])
def test_a_tilted_plane_gives_one_minus_cos_theta_everywhere(theta_deg):
    W, H = 37, 23
    theta = math.radians(theta_deg)
    D, A, N, cam, n = NR.plane_case(W, H, theta=theta)
    out3, S, sup = NR.loss(torch.tensor(D), torch.tensor(A), torch.tensor(N), *cam, 0.5, 0.1, float("inf"), 2.0)
    assert S == (W - 2) * (H - 2) and bool(sup.all())
    want = 1.0 - math.cos(theta)
    assert abs(float(out3[1]) - want) <= 1e-12 and abs(float(out3[0]) - 2.0 * want) <= 2e-12
    assert float(out3[2]) == S / (W * H)


def test_the_depth_normal_of_a_plane_faces_the_camera():
    # c = b x a, not a x b: with the plane's own (camera-facing) normal rho is 0, with its opposite it is 2
    D, A, N, cam, n = NR.plane_case(16, 17)
    assert n[2] < 0
    lo = NR.loss(torch.tensor(D), torch.tensor(A), torch.tensor(N), *cam, 0.5, 0.1, float("inf"), 1.0)[0]
    hi = NR.loss(torch.tensor(D), torch.tensor(A), torch.tensor(-N), *cam, 0.5, 0.1, float("inf"), 1.0)[0]
    assert abs(float(lo[1])) <= 1e-12 and abs(float(hi[1]) - 2.0) <= 1e-12


def test_the_principal_point_matters():
    # cx = W / 2 for (W - 1) / 2 tilts every ray: the plane's own normal no longer gives rho = 0
    W, H = 37, 23
    D, A, N, cam, _ = NR.plane_case(W, H, normal=(0.6, -0.4, -1.0))
    off = (cam[0], cam[1], W / 2.0, cam[3])
    good = NR.loss(torch.tensor(D), torch.tensor(A), torch.tensor(N), *cam, 0.5, 0.1, float("inf"), 1.0)[0]
    out3 = NR.loss(torch.tensor(D), torch.tensor(A), torch.tensor(N), *off, 0.5, 0.1, float("inf"), 1.0)[0]
    assert abs(float(good[1])) <= 1e-12 and float(out3[1]) > 5e-6


def test_every_interior_pixel_of_an_all_valid_image_is_supervised():
    for W, H in NR.SHAPES + [(9, 7)]:
        D, A, N, cam = NR.loss_case(W, H)
        _, _, _, S, sup = NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, float("inf"), 1.0)
        assert S == (W - 2) * (H - 2) and sup.shape == (H - 2, W - 2)
    for W, H in ((2, 2), (1, 7), (7, 1)):
        D, A, N, cam = NR.loss_case(W, H)
        out3, gd, ga, S, _ = NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, float("inf"), 1.0)
        assert S == 0 and not out3.any() and not gd.any() and not ga.any()


# ---- the loss: gates -------------------------------------------------------------------------------------------------------
def test_gates_remove_the_predicted_pixels():
    W, H = 16, 17
    D, A, N, cam = NR.loss_case(W, H)
    full = (W - 2) * (H - 2)
    # one pixel below acc_min: itself and its four neighbours
    A1, D1 = A.copy(), D.copy()
    A1[8, 5] = 0.3
    D1[8, 5] = D[8, 5] / A[8, 5] * 0.3
    _, _, _, S, sup = NR.loss_and_grads(D1, A1, N, cam, 0.5, 0.1, float("inf"), 1.0)
    gone = {(y + 1, x + 1) for y, x in zip(*np.nonzero(~sup))}
    assert S == full - 5 and gone == {(8, 5), (7, 5), (9, 5), (8, 4), (8, 6)}
    # a NaN silhouette is an invalid pixel, confined to the same five
    A2 = A.copy()
    A2[8, 5] = np.nan
    out3, gd, ga, S, _ = NR.loss_and_grads(D, A2, N, cam, 0.5, 0.1, float("inf"), 1.0)
    assert S == full - 5 and np.isfinite(out3).all() and np.isfinite(gd).all() and np.isfinite(ga).all()
    # normal_min
    N3 = N.copy()
    N3[:, 3, 4] *= 0.05 / np.linalg.norm(N3[:, 3, 4]) * A[3, 4]          # |N| / A = 0.05 < 0.1
    assert NR.loss_and_grads(D, A, N3, cam, 0.5, 0.1, float("inf"), 1.0)[3] == full - 1
    assert NR.loss_and_grads(D, A, N3, cam, 0.5, 0.04, float("inf"), 1.0)[3] == full


def test_a_depth_step_removes_the_pixels_either_side_of_it():
    W, H = 16, 17
    D, A, N, cam, _ = NR.plane_case(W, H)                 # z within [3.4, 4.8]: neighbours differ by far less than 5 %
    D = D.copy()
    D[:, 9:] *= 1.5                                          # a step between columns 8 and 9
    _, _, _, S, sup = NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, 0.05, 1.0)
    want = np.ones((H - 2, W - 2), bool)
    want[:, 7:9] = False                                     # interior columns 8 and 9 see the step
    assert np.array_equal(sup, want) and S == (W - 4) * (H - 2)
    assert NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, float("inf"), 1.0)[3] == (W - 2) * (H - 2)


# ---- the loss: gradients ---------------------------------------------------------------------------------------------------
def test_gradcheck_of_the_float64_loss():
    W, H = 9, 7
    D, A, N, cam = NR.loss_case(W, H)
    Dt = torch.tensor(D, dtype=torch.float64, requires_grad=True)
    At = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    Nt = torch.tensor(N, dtype=torch.float64)
    for jump in (float("inf"), 0.2):
        fn = lambda d, a: NR.loss(d, a, Nt, *cam, 0.5, 0.1, jump, 0.7)[0][0]   # noqa: E731
        assert torch.autograd.gradcheck(fn, (Dt, At), eps=1e-7, atol=1e-7, rtol=1e-5)


def test_the_loss_depends_on_depth_over_acc_only():
    # dL/dA = -dL/dD * D / A: scaling D and A together changes nothing
    D, A, N, cam = NR.loss_case(16, 17)
    out3, gd, ga, _, _ = NR.loss_and_grads(D, A, N, cam, 0.5, 0.1, float("inf"), 0.7)
    z = D.astype(np.float64) / A.astype(np.float64)
    np.testing.assert_allclose(ga, -gd * z, rtol=1e-12, atol=1e-18)
    assert np.abs(gd).max() > 0


def test_loss_yardstick_stays_within_the_recorded_ratios():
    wo = wg = 0.0
    for W, H in NR.SHAPES:
        for seed in NR.SEEDS:
            D, A, N, cam = NR.loss_case(W, H, seed)
            for jump in NR.JUMPS:
                kw = dict(NR.CASE_KW, jump_rel=jump)
                r64 = NR.loss_and_grads(D, A, N, cam, **kw)
                r32 = NR.loss_and_grads(D, A, N, cam, dt=torch.float32, **kw)
                assert r64[3] == r32[3]                       # no gate sits within float32 rounding of its threshold
                wo = max(wo, NR.rel(r32[0], r64[0]))
                wg = max(wg, NR.grad_ratio(r32[1], r64[1]), NR.grad_ratio(r32[2], r64[2]))
    print("float32 loss worst: out3 %.3e  gradients %.3e" % (wo, wg))
    assert 0.5 * NR.YARD_OUT3 <= wo <= NR.YARD_OUT3
    assert 0.5 * NR.YARD_GRADS <= wg <= NR.YARD_GRADS
