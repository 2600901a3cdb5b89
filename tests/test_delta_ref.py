"""CPU tests of tests/delta_ref.py (the restatement of the delta-depth term the GPU tests hold csrc/delta.hip to) and of
loss.delta_pose: two independent float64 evaluations agree, gradcheck, closed forms, the pose convention, and -- what
licenses the 1 % cap of tests/test_gpu_delta.py -- the fragile share and the float32 restatement on every GPU-test
input."""
import numpy as np
import pytest
import torch

import delta_ref as D
import gs_livm_amd as G

F64 = torch.float64


@pytest.mark.parametrize("case", [c for c in D.CASE_NAMES if not c.startswith("512")])
def test_two_float64_evaluations_agree(case):
    x = D.inputs(case)
    a, e = D.restatement(*D._args(x)), D.reference(case)["truth"]
    keep = D.reference(case)["keep"]
    for k in ("loss", "mean_gap", "share"):
        assert abs(float(a[k]) - float(e[k])) <= 1e-12, k
    assert float((a["warped"] - e["warped"]).abs().max()) <= 1e-12 * float(e["warped"].abs().max())
    for k in ("grad_src", "grad_ref"):   # (the analytic gradient against autograd, away from the kinks)
        d = torch.where(keep[k], (a[k] - e[k]).abs(), torch.zeros_like(a[k]))
        assert float(d.max()) <= 1e-12 * max(1.0, float(e[k].abs().max())), k
        assert float(e[k].abs().max()) > 0 or case == "2x2", k


def _smooth(H=9, W=7):
    v, u = np.mgrid[0:H, 0:W]
    ds = 4.0 + 0.3 * np.sin(0.5 * u + 0.113) + 0.2 * np.cos(0.4 * v + 0.271)
    dr = ds + 0.37 + 0.05 * np.sin(0.3 * u * v + 0.1)
    ones = np.ones((H, W))
    Ks, Kr, iKs = D.intrinsics(H, W)
    return ds, ones, dr, ones, iKs, Kr, D.pose("rpy")


def test_gradcheck_smooth_case():
    ds, a_s, dr, a_r, iK, Kr, T = _smooth()
    e = D.explicit(ds, a_s, dr, a_r, iK, Kr, T, 0.2)
    # away from the kinks: no sample coordinate near an integer, no |a - b| near 0
    fr = lambda v: (v - torch.round(v)).abs()  # noqa: E731
    ins = e["inside"]
    assert float(torch.where(ins, torch.minimum(fr(e["Xs"]), fr(e["Ys"])), torch.ones_like(e["Xs"])).min()) > 1e-3
    assert float((e["a"] - e["b"]).abs().min()) > 1e-3 and bool(ins.any())
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=F64)  # noqa: E731
    T4 = torch.eye(4, dtype=F64)
    T4[:3] = t(T)
    d_s = t(ds)[None].clone().requires_grad_(True)
    d_r = t(dr)[None].clone().requires_grad_(True)
    fn = lambda x, y: D.forward_ops(x, t(a_s)[None], y, t(a_r)[None], t(iK), t(Kr), T4, 0.2)[0]  # noqa: E731
    assert torch.autograd.gradcheck(fn, (d_s, d_r), eps=1e-6, atol=1e-9, rtol=1e-6)
    # and the analytic gradient of explicit() is that gradient
    auto = D.restatement(ds, a_s, dr, a_r, iK, Kr, T, 0.2)
    for k in ("grad_src", "grad_ref"):
        assert float((auto[k] - e[k]).abs().max()) <= 1e-12 and float(e[k].abs().max()) > 0


def test_identity_pose_gives_zero_loss():
    H, W = 11, 13
    rng = np.random.default_rng(0)
    ds = rng.uniform(2.0, 8.0, (H, W))
    K = D.intrinsics(H, W)[0].astype(np.float64)
    T = np.eye(4)[:3]
    ones = np.ones((H, W))
    for fn in (D.restatement, D.explicit):
        r = fn(ds, ones, ds.copy(), ones, np.linalg.inv(K), K, T, 0.2)
        assert abs(float(r["loss"])) <= 1e-12
        assert float((r["warped"] - torch.as_tensor(ds)).abs().max()) <= 1e-12


def test_half_pixel_shift_of_constant_depth():
    """Constant depth d and t_rel = (d / (2 fx), 0, 0): X = u + 1/2, so out is the mean of the horizontal neighbours of
    Z' = d, with zero padding beyond the last column."""
    H, W, d, fx = 6, 9, 4.0, 8.0
    K = np.array([[fx, 0, 4.0], [0, 10.0, 2.5], [0, 0, 1]])
    T = np.eye(4)[:3].copy()
    T[0, 3] = d / (2 * fx)
    ds, ones = np.full((H, W), d), np.ones((H, W))
    want = np.full((H, W), d)
    want[:, -1] = d / 2
    for fn in (D.restatement, D.explicit):
        r = fn(ds, ones, ds, ones, np.linalg.inv(K), K, T, 1.0)
        assert float((r["warped"] - torch.as_tensor(want)).abs().max()) <= 1e-12
        # gap: 0 inside, |2/d - 1/d| in the last column
        assert abs(float(r["mean_gap"]) - (1.0 / d) / W) <= 1e-12


def test_delta_pose_is_the_references_transposed_product():
    rng = np.random.default_rng(5)

    def rot(v):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)) + v)
        return q * np.sign(np.linalg.det(q))
    Rs, Rr = rot(0.0), rot(1.0)
    ts, tr = rng.standard_normal(3), rng.standard_normal(3)

    def hand(Rs, Rr, transpose):
        Ts, Tr = np.eye(4), np.eye(4)
        Ts[:3, :3], Ts[:3, 3] = (Rs.T if transpose else Rs), ts
        Tr[:3, :3], Tr[:3, 3] = (Rr.T if transpose else Rr), tr
        # inverse of a rigid transform, written out
        Ti = np.eye(4)
        Ti[:3, :3] = Ts[:3, :3].T
        Ti[:3, 3] = -Ts[:3, :3].T @ ts
        return (Tr @ Ti)[:3]
    got = G.delta_pose(Rs, ts, Rr, tr)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4)
    assert np.abs(got.numpy() - hand(Rs, Rr, True)).max() <= 2.0 ** -23 * 4
    # forgetting the transposition is a different matrix, far outside that tolerance
    assert np.abs(got.numpy() - hand(Rs, Rr, False)).max() > 1e-2
    # tensors, float32 inputs and nested lists are accepted alike
    again = G.delta_pose(torch.as_tensor(Rs), list(ts), Rr.tolist(), torch.as_tensor(tr))
    assert torch.equal(again, got)


@pytest.mark.parametrize("case", D.CASE_NAMES)
def test_fragile_share_and_float32_restatement_on_gpu_inputs(case):
    """The fragile set stays at or below 1 % on every input of tests/test_gpu_delta.py, and the float32 restatement
    -- the reference's own arithmetic -- stays inside every bar on the kept pixels."""
    ref = D.reference(case)
    assert ref["fragile_share"] <= 0.01, ref["fragile_share"]
    got = {k: ref["f32"][k].to(F64) for k in ("warped", "grad_src", "grad_ref", "loss", "mean_gap", "share")}
    r = D.ratios(got, ref)
    print(case, "fragile share %.4f" % ref["fragile_share"], "float32 |d| / bar:", {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    e = ref["truth"]
    if not case.startswith(("2x2", "5x3")):
        assert float(e["grad_src"].abs().max()) > 0 and float(e["grad_ref"].abs().max()) > 0
        assert 0.3 < float(e["share"]) < 1.0


def test_inputs_exercise_what_they_claim():
    for case in D.CASE_NAMES:
        x, e = D.inputs(case), D.reference(case)["truth"]
        outside = float((~e["inside"]).to(F64).mean())
        if "shift" in case:
            assert 0.2 < outside < 0.45, (case, outside)
        if "backward" in case:
            assert int((e["Nn"][2] <= 0).sum()) > 0, case
        if x["H"] >= 16:
            assert (x["depth_src"] == 0).any() and (x["depth_ref"] == np.float32(0.01)).any()
            assert (x["acc_src"] < 0.5).any() and (x["acc_ref"] < 0.5).any()
            if "rpy" in case:   # unmasked holes that land inside: the many-to-one scatter has work to do
                hole = torch.as_tensor(x["depth_src"] == 0).reshape(-1)
                assert int((hole & (e["u"] != 0)).sum()) > 4, case
    assert all(abs(v) > 1e-3 for v in D.pose("rpy")[:, :3].reshape(-1))
