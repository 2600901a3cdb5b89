"""CPU anchor of tests/optim_ref.py, the float64 reference csrc/optimizer.hip is held to (test_gpu_optim_ref64.py):
its Adam against torch.optim.Adam, its activations against gradcheck and the clamped branch of normalize, and the bar
formula exercised on the float32 / float64 pair of the reference itself."""
import json

import pytest
import torch

import optim_ref as R

U64 = 2.0 ** -52


@pytest.mark.parametrize("eps,lr", [(1e-15, 1e-3), (1e-8, 2.5e-2)])
def test_adam_float64_matches_torch_optim_adam_over_60_steps(eps, lr):
    """adam_step (the C++ torch::optim::Adam formula) against torch.optim.Adam on float64 CPU tensors, 60 steps,
    gradients walking over the decades 1e-12 ... 1e8 with 10 % exact zeros.

    The two differ only in roundings (Python's Adam uses lerp_ and addcmul_).  Bars, per element:
      exp_avg     3 roundings a step (constant, multiply, add), each at most 2^-52 max_t |g_t| since |m| <= max |g|, and a
                  past error decays by beta1 a step: 3 / (1 - beta1) = 30 roundings of max_t |g_t|;
      exp_avg_sq  4 a step, decaying by beta2: 4 / (1 - beta2) = 4000 roundings of max_t g_t^2;
      p           the update inherits the relative error of exp_avg (30) and half that of exp_avg_sq through the root
                  (2000), plus its own root, divide by sqrt(bc2), add eps, divide, multiply by step_size, subtract: 6;
                  N = 30 + 2000 + 6 = 2036 roundings of 2^-52 on |p| + sum |updates so far|."""
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(257, 3, generator=gen, dtype=torch.float64)
    p0[0] = 0.0
    p0[1] *= 1e-9
    a = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([a], lr=lr, betas=R.BETAS, eps=eps)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    moved, gmax = torch.zeros_like(p0), torch.zeros_like(p0)
    decade = -12 + 20 * torch.rand(p0.shape, generator=gen, dtype=torch.float64)
    N = 3 / (1 - R.BETAS[0]) + 0.5 * 4 / (1 - R.BETAS[1]) + 6
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step in range(1, 61):
        decade = (decade + 3 * torch.randn(p0.shape, generator=gen, dtype=torch.float64)).clamp(-12, 8)
        g = 10.0 ** decade * (torch.randint(0, 2, p0.shape, generator=gen).double() * 2 - 1)
        g = torch.where(torch.rand(p0.shape, generator=gen) < 0.1, torch.zeros_like(g), g)
        a.grad = g.clone()
        opt.step()
        new, m, v = R.adam_step(p, g, m, v, lr, step, eps=eps)
        moved += (new - p).abs()
        p = new
        gmax = torch.maximum(gmax, g.abs())
        st = opt.state[a]
        for name, got, ref, bar in (("p", p, a.detach(), N * U64 * (p.abs() + moved)),
                                    ("m", m, st["exp_avg"], 3 / (1 - R.BETAS[0]) * U64 * gmax),
                                    ("v", v, st["exp_avg_sq"], 4 / (1 - R.BETAS[1]) * U64 * gmax * gmax)):
            err = (got - ref).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp(min=1e-300))
            worst[name] = max(worst[name], float(ratio.max()))
            assert bool((err <= bar).all()), "%s at step %d: %.3g of its bar" % (name, step, float(ratio.max()))
    print(json.dumps(dict(what="adam64 vs torch.optim.Adam", eps=eps, lr=lr, worst_over_bar=worst)))
    assert float(moved.min()) > 0.0


def test_activations_pass_gradcheck_away_from_the_clamp():
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_(True)  # noqa: E731
    assert torch.autograd.gradcheck(R.activations, (r(5, 3), r(5, 4), r(5, 1) * 3, r(5, 1, 3), r(5, 3, 3)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_clamped_branch_of_normalize(dtype):
    """|q| < 1e-12 (and q = 0): y = q / 1e-12 and autograd hands back g * 1e12; just above the clamp the projection."""
    q = torch.tensor([[3e-13, -4e-13, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [3e-12, -4e-12, 0.0, 0.0]], dtype=dtype)
    g = torch.tensor([[1.0, 2.0, -3.0, 0.5]] * 3, dtype=dtype)
    raw = dict(scaling=torch.zeros(3, 3), rotation=q, opacity=torch.zeros(3, 1), f_dc=torch.zeros(3, 1, 3),
               f_rest=torch.zeros(3, 0, 3))
    ups = (torch.zeros(3, 3), g, torch.zeros(3, 1), torch.zeros(3, 1, 3))
    act, grads = R.activations_backward(raw, ups, dtype)
    tol = 4 * (2.0 ** -52 if dtype == torch.float64 else R.EPS32)
    torch.testing.assert_close(act[1][:2].double(), q[:2].double() * 1e12, rtol=tol, atol=0)
    torch.testing.assert_close(grads["rotation"][:2].double(), g[:2].double() * 1e12, rtol=tol, atol=0)
    y = torch.tensor([0.6, -0.8, 0.0, 0.0], dtype=torch.float64)
    want = (g[2].double() - y * (y * g[2].double()).sum()) / 5e-12
    torch.testing.assert_close(grads["rotation"][2].double(), want, rtol=8 * tol, atol=8 * tol * 1e12)


GENERATORS = [(P, M, step, eps) for P, M in ((1, 1), (5, 2), (257, 4), (1025, 9), (129, 16), (20011, 1))
              for step, eps in ((1, 1e-15), (2, 1e-8), (1000, 1e-15), (30000, 1e-8))]


@pytest.mark.parametrize("P,M,step,eps", GENERATORS)
def test_float32_restatement_stays_inside_the_floor_and_the_drop_cap(P, M, step, eps):
    """The bar formula without a GPU: the float32 restatement is Torch's arithmetic in another order of operations, so
    the rounding counts K must cover it too -- its distance from float64 stays inside the floor K 2^-23 magnitude alone
    on every judged element, and the generator leaves at most 0.1 % of the elements unjudgeable."""
    case = R.make_case(P, M, seed=3, step=step)
    hyper = dict(step=step, eps=eps)
    r64, r32 = R.model_step_ref(case, torch.float64, **hyper), R.model_step_ref(case, torch.float32, **hyper)
    ok = R.judgeable(case, r64, **hyper)
    assert R.dropped_fraction(ok) <= R.DROP_CAP, R.dropped_fraction(ok)
    fl = R.floors(case, r64, **hyper)
    bar = R.bars(case, r64, r32, **hyper)
    for a in fl:
        for k in fl[a]:
            e, b = bar[a][k]
            assert bool((b >= fl[a][k]).all()) and bool((b >= 2 * e).all())
    res = R.worst_ratios({a: r32[a] for a in fl}, r64, {a: {k: (bar[a][k][0], fl[a][k]) for k in fl[a]} for a in fl}, ok)
    worst = {k: round(v[3], 4) for k, v in res.items()}
    print(json.dumps(dict(what="float32 restatement over floor", P=P, M=M, step=step, eps=eps,
                          dropped=R.dropped_fraction(ok), worst=worst)))
    for k, v in res.items():
        assert v[3] <= 1.0, "%s: float32 Torch is at %.3g of the floor" % (k, v[3])
    if P >= 257:   # the generator reaches what it promises
        qn = case["p"]["rotation"].double().norm(dim=1)
        assert bool((qn == 0).any()) and bool(((qn > 0) & (qn < 1e-12)).any()) and bool((qn > 1e3).any())
        assert bool((case["p"]["opacity"].abs() > 12).any())
        dead = case["culled"]
        assert bool(dead.any()) and all(not bool(case["ups"][k][dead].any()) for k in case["ups"])


def test_every_generator_of_the_gpu_module_stays_inside_the_drop_cap():
    """Every (P, M, step, eps, seed) test_gpu_optim_ref64.py feeds the kernels, the large model aside (held there): at
    most 0.1 % of a case may be unjudgeable -- in a small case, not one element."""
    configs = [(P, M) + R.grid_hyper(i) + (1,) for i, (M, P) in enumerate(R.GRID)]
    configs += [(257, M, step, eps, 2) for M in (1, 4) for step in R.STEPS for eps in R.EPSES]
    configs += [(1025, M, step, 1e-15, 5) for M, step in ((1, 1), (4, 1), (4, 10), (9, 1000))]
    configs += [(P, M, 10, 1e-8, 7) for P, M in ((3, 2), (1, 1), (2, 2), (4, 4), (63, 4), (257, 1), (2, 1), (1, 2), (2, 4),
                                                 (3, 1), (64, 2), (5, 1), (129, 9))]
    worst = 0.0
    for P, M, step, eps, seed in configs:
        case = R.make_case(P, M, seed=seed, step=step)
        r64 = R.model_step_ref(case, torch.float64, step=step, eps=eps)
        frac = R.dropped_fraction(R.judgeable(case, r64, step=step, eps=eps))
        worst = max(worst, frac)
        assert frac <= R.DROP_CAP, (P, M, step, eps, seed, frac)
    print(json.dumps(dict(what="drop cap over the GPU module's generators", cases=len(configs), worst=worst)))
