"""CPU tests of the references of the camera pose gradient (tests/pose_ref.py) and of se3_exp.

The xi-leaf gradient against central differences; the closed form against the xi-leaf gradient on every end-to-end case;
dL/drho against ref64's own dL_dmeans3D; se3_exp; the half-bar condition of the float32 yardstick on every case the GPU
tests run; the mutant table; the pose-refinement loop of tests/test_gpu_pose.py in float64."""
import numpy as np
import pytest
import torch

import depth_ref as DR
import gs_livm_amd as G
import pose_ref as PR
import ref64 as R
from oracle import oracle as O

F32_GRADS = ("dL_dmeans2D", "dL_dconic", "dL_dmeans3D", "dL_ddepths")


def _as_f32(a):
    """the arrays as a float32 backward hands them over"""
    return {**a, **{k: (None if a[k] is None else np.asarray(a[k], np.float32)) for k in F32_GRADS}}


def _case_arrays(name, mix):
    sc, fr, up, r, g = PR.render64_pose(name, mix)
    return PR.arrays_of(sc, fr.radii, r), g, r, sc, fr


def test_xi_gradient_matches_central_differences():
    """departures off: the straight-through terms are not derivatives of anything a difference quotient sees"""
    sc, _ = PR.scene("P300_70x50")
    fr = PR.frame("P300_70x50")
    vis = np.flatnonzero(fr.radii > 0)
    rng = np.random.default_rng(0)
    n = len(vis)
    g2 = {"ndc": PR._t(rng.normal(size=(n, 2))), "conic": PR._t(rng.normal(size=(n, 3))),
          "color": PR._t(rng.normal(size=(n, 3))), "depth": PR._t(rng.normal(size=n))}
    g = PR.xi_gradient(sc, vis, fr.clamped, g2, departures=False)
    h = 1e-6
    for k in range(6):
        e = torch.zeros(6, dtype=R.F64)
        e[k] = h
        with torch.no_grad():
            d = (PR.pose_loss(sc, vis, fr.clamped, g2, e, False) - PR.pose_loss(sc, vis, fr.clamped, g2, -e, False)) / (2 * h)
        assert abs(float(d) - g[k]) <= 1e-6 * max(1.0, float(np.abs(g).max())), (k, float(d), g[k])
    assert np.abs(g).min() > 0


@pytest.mark.parametrize("mix", PR.MIXES)
@pytest.mark.parametrize("name", PR.CASES)
def test_closed_form_matches_the_xi_leaf_gradient(name, mix):
    a, g, r, sc, fr = _case_arrays(name, mix)
    closed, bar = PR.pose_gradient64(a), PR.bar(a)
    # (what separates them is the float32 projmatrix the closed form is handed against the exact view . P: counted in the bar)
    assert (np.abs(closed - g) <= 0.05 * bar).all(), np.abs(closed - g) / bar
    # dL/drho = R sum_i dL_dmean3D_i with ref64's own gradients
    Rm = np.asarray(sc["viewmatrix"], np.float64)[:3, :3].T
    rho = Rm @ np.asarray(r["dL_dmeans3D"], np.float64).sum(0)
    assert (np.abs(rho - g[:3]) <= 0.05 * bar[:3]).all()
    # the float32 yardstick stays within half the bar (the condition the bar comes with)
    y = PR.yardstick32(_as_f32(a))
    assert (np.abs(y - closed) <= 0.5 * bar).all(), np.abs(y - closed) / bar


def test_yardstick_within_half_the_bar_on_the_array_cases():
    """every input tests/test_gpu_pose.py hands the reduction as a pure function of arrays"""
    cases = [dict(P=P, seed=100 + P, tail_gain=1024.0 if P > 4096 else 1.0)
             for P in (1, 7, 63, 64, 65, 255, 256, 257, PR.ROWS_PER_BLOCK * PR.FINISH_THREADS + 1)]
    cases += [dict(P=P, seed=100 + P, hidden_frac=0.4) for P in (65, 257, 3 * 256 + 7)]
    cases += [dict(P=257, seed=7, **kw) for kw in (dict(), dict(precomp=True), dict(depth=False),
                                                   dict(precomp=True, depth=False))]
    worst = 0.0
    for kw in cases:
        a = PR.random_arrays(kw.pop("P"), kw.pop("seed"), **kw)
        ratio = np.abs(PR.yardstick32(a) - PR.pose_gradient64(a)) / PR.bar(a)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 0.5).all(), (kw, ratio)
    print("yardstick32: worst |d| / bar over the array cases %.4f" % worst)


def test_se3_exp():
    gen = torch.Generator().manual_seed(1)
    for scale in (0.0, 1e-9, 1e-3, 0.3, 0.499, 0.501, 1.5, 3.0):
        xi = torch.randn(6, generator=gen, dtype=torch.float64)
        xi[3:] *= scale / xi[3:].norm()
        E = G.se3_exp(xi)
        K = torch.zeros(4, 4, dtype=torch.float64)
        p = xi[3:]
        K[:3, :3] = torch.tensor([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        K[:3, 3] = xi[:3]
        assert float((E - torch.linalg.matrix_exp(K)).abs().max()) <= 1e-14
        assert float((E[:3, :3] @ E[:3, :3].T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14
        assert abs(float(torch.linalg.det(E[:3, :3])) - 1.0) <= 1e-14
        assert float((E @ G.se3_exp(-xi) - torch.eye(4, dtype=torch.float64)).abs().max()) <= 1e-14
        assert torch.equal(E[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
        E32 = G.se3_exp(xi.float())
        assert E32.dtype == torch.float32 and float((E32.double() - E).abs().max()) <= 4e-7 * max(1.0, float(E.abs().max()))
    # differentiable at xi = 0: the generators
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    J = torch.autograd.functional.jacobian(G.se3_exp, xi)
    assert torch.isfinite(J).all() and float(J[0, 3, 0]) == 1.0 and float(J[2, 1, 3]) == 1.0 and float(J[1, 2, 3]) == -1.0
    with pytest.raises(ValueError):
        G.se3_exp(torch.zeros(7))


# mutant -> the case meant to catch it: an end-to-end case (name, mix) or the arguments of pose_ref.random_arrays
MUTANT_CASES = {
    "no_cov": ("P300_70x50", "all"),
    "cov_sign": ("P300_70x50", "all"),
    "no_depth": ("P300_70x50", "depth_only"),
    "sh_in_rot": dict(P=257, seed=357),            # dL_dmean3D unrelated to dm_geo; (the SH part of a real frame's
                                                   # dL_dmean3D is small against the geometric part: measured below)
    "view_T": ("pose_rpy", "all"),
    "fx_for_fy": ("wide_y", "all"),
    "no_scale_modifier": ("scale_modifier", "all"),
    "no_xymul": ("jacobian_clamp", "all"),
    "rho_world": ("pose_rpy", "all"),
    "drop_last_block": dict(P=257, seed=357),
    "drop_beyond_finish": dict(P=PR.ROWS_PER_BLOCK * PR.FINISH_THREADS + 1,
                               seed=100 + PR.ROWS_PER_BLOCK * PR.FINISH_THREADS + 1, tail_gain=1024.0),
}


def test_every_mutant_moves_the_result_beyond_the_bar():
    assert set(MUTANT_CASES) == set(PR.MUTANTS)
    table = {}
    for mutant, case in MUTANT_CASES.items():
        a = _case_arrays(*case)[0] if isinstance(case, tuple) else PR.random_arrays(**case)
        ratio = np.abs(PR.pose_gradient64(a, mutant) - PR.pose_gradient64(a)) / PR.bar(a)
        table[mutant] = float(ratio.max())
        assert ratio.max() > 1.0, (mutant, case, ratio)
    print("mutant: largest move / bar", {k: round(v, 1) for k, v in table.items()})
    # view_T is invisible under a yaw-only camera (tests/poses.py): the reason its case is a dense pose
    a = _case_arrays("P300_70x50", "all")[0]
    V = np.asarray(a["viewmatrix"])
    assert V[0, 1] == 0 and V[1, 0] == 0 and V[1, 2] == 0 and V[2, 1] == 0
    # sh_in_rot on a real frame with SH degree 3: recorded, not asserted (it stays below the bar of the reduction)
    moved = np.abs(PR.pose_gradient64(a, "sh_in_rot") - PR.pose_gradient64(a)) / PR.bar(a)
    print("sh_in_rot on P300_70x50 / all: move / bar", np.round(moved, 3))


# ---- the refinement loop of tests/test_gpu_pose.py in float64 --------------------------------------------------------
def _scene_at(sc0, Tcw):
    view = Tcw.T
    cam = dict(viewmatrix=view.numpy().astype(np.float32),
               projmatrix=(view @ PR.projection_of(sc0)).numpy().astype(np.float32),
               campos=(-(Tcw[:3, :3].T @ Tcw[:3, 3])).numpy().astype(np.float32))
    return dict(sc0, **cam)


def _images(sc):
    O.set_threads(min(O.max_threads(), 16))
    fr = O.forward(sc)
    out = R.render(sc, fr)
    return fr, [torch.from_numpy(out[k]) for k in ("out_color", "out_depth", "out_acc")]


def _loop64(step, steps=10):
    sc0, _ = PR.scene("P300_70x50")
    T_true = PR._t(sc0["viewmatrix"]).T
    _, (target, target_depth, target_acc) = _images(sc0)
    lidar = torch.where(target_acc >= 0.5, target_depth / target_acc.clamp(min=1e-6), torch.zeros_like(target_depth))
    off = torch.tensor([0.02 / 3 ** 0.5] * 3 + [np.deg2rad(1.0) / 3 ** 0.5] * 3, dtype=R.F64)
    Tcw = G.se3_exp(off) @ T_true

    def error():
        D = Tcw @ torch.linalg.inv(T_true)
        return float(D[:3, 3].norm() + torch.arccos(((torch.trace(D[:3, :3]) - 1.0) * 0.5).clamp(-1.0, 1.0)))

    def loss_and_grads(sc):
        fr, imgs = _images(sc)
        color, depth, acc = (x.clone().requires_grad_(True) for x in imgs)
        sup = (lidar > 0) & (acc.detach() >= 0.5)
        loss = (color - target).abs().mean() + ((depth / acc.clamp(min=1e-6) - lidar).abs() * sup).sum() / sup.sum().clamp(min=1)
        gs = torch.autograd.grad(loss, [color, acc, depth], allow_unused=True)
        return fr, float(loss.detach()), [torch.zeros_like(x) if g is None else g for g, x in zip(gs, (color, acc, depth))]
    xi = torch.zeros(6, dtype=R.F64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=step)
    err0 = error()
    loss0 = None
    for _ in range(steps):
        sc = _scene_at(sc0, Tcw)
        fr, loss, (g_c, g_a, g_d) = loss_and_grads(sc)
        loss0 = loss if loss0 is None else loss0
        r = DR.render64(sc, fr, g_c.numpy(), g_a.numpy(), g_d.numpy())
        vis = np.flatnonzero(fr.radii > 0)
        xi.grad = torch.from_numpy(PR.xi_gradient(sc, vis, fr.clamped, PR.upstream2d(r, vis)))
        opt.step()
        with torch.no_grad():
            Tcw = G.se3_exp(xi.detach()) @ Tcw
            xi.zero_()
    _, loss1, _ = loss_and_grads(_scene_at(sc0, Tcw))
    return loss0, loss1, err0, error()


def test_refinement_loop_in_float64():
    """The loop of test_gpu_pose.py's refinement test -- photometric L1 + the LiDAR-style depth L1 on depth / acc, ten
    Adam steps on xi, a retraction after each -- with the float64 pose gradient.  The step the GPU test uses passes with
    room on both sides: so do half and twice of it."""
    for step in (5e-4, 1e-3, 2e-3):
        loss0, loss1, err0, err1 = _loop64(step)
        print("step %g: loss %.4f -> %.4f, pose error %.5f -> %.5f" % (step, loss0, loss1, err0, err1))
        assert loss1 < loss0 and err1 < err0, step
