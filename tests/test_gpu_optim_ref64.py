"""GPU tests of the optimiser tail (csrc/optimizer.hip: k_activate, k_sh_move, k_activate_backward, k_adam, k_model_step,
k_sh_step) against the float64 restatement in tests/optim_ref.py, on every code path.

What is compared, per element, from identical float32 inputs and over ONE step (no trajectory to diverge): the
activations, the raw-space gradients, exp_avg, exp_avg_sq, the update p_new - p_old (formed in float64 from the two
float32 values; the parameter alone would hide it: the update is ~1e-3 of |p|), and the activations of the updated
parameters.  The bar of every quantity is max(2 e_ref, K 2^-23 magnitude); K, the magnitudes and what cannot be judged
are derived in the docstring of optim_ref.py, before any kernel ran, and are not fitted to what the kernels return.
Every figure is printed as a JSON line before it is asserted; the worst ratios measured on an MI355X are in DESIGN.md
section 2.

Exact assertions (no bar): an element with g == 0, m == 0, v == 0 keeps p, m, v bit for bit; zero_grads zeroes exactly
the consumed gradients and zero_grads = 0 leaves them; SH values pass through k_sh_move bit for bit in both directions;
shs_out holds the updated SH leaves bit for bit; the guard floats either side of every (misaligned) view keep their NaN
pattern; two runs are bitwise equal.

Which branch runs is decided by the pointers.  `_model_step_branches` / `_adam_branches` restate the conditions of
launch_model_step / k_model_step / launch_adam / launch_sh_move from the pointers handed in, and every case asserts
the branch it is there for.  The 64-bit index branches (numel > 0xFFFFFFFF in k_sh_move, > 0xFFFFFFF0 in k_model_step)
need tensors beyond 16 GB and stay out.
"""
import ctypes as C
import functools
import json

import pytest
import torch

import gs_livm_amd as G
import optim_ref as R
from arena import Arena, offsets

pytestmark = pytest.mark.gpu
GRID, P_LARGE = R.GRID, R.P_LARGE


# ---- which branch the pointers select (launch_model_step / k_model_step / launch_adam / launch_sh_move restated) ----
def _al(*ptrs):
    return all((p or 0) % 16 == 0 for p in ptrs)


def _model_step_branches(P, M, ptr, outs):
    o = (lambda k: ptr("o." + k)) if outs else (lambda k: None)
    extra = dict(xyz=(ptr("g.xyz"),), f_dc=(ptr("g.shs"), o("shs")), f_rest=(), scaling=(ptr("g.scales"), o("scales")),
                 rotation=(ptr("g.rotations"), o("rotations")), opacity=(ptr("g.opacities"), o("opacities")))
    aligned = {k: _al(ptr("p." + k), ptr("m." + k), ptr("v." + k), *extra[k]) for k in R.GROUPS}
    numel = dict(xyz=3 * P, f_dc=3 * P, f_rest=3 * (M - 1) * P, scaling=3 * P, rotation=4 * P, opacity=P)
    staged = M > 1 and P > 0 and aligned["f_dc"] and aligned["f_rest"] and 64 * 3 * M * 4 <= 64 * 1024
    br = set()
    if staged:
        br.add("k_sh_step")
    for k in R.GROUPS:
        n = numel[k]
        if n == 0 or (staged and k in ("f_dc", "f_rest")):
            continue
        if k == "rotation":
            br.add("quat16" if aligned[k] else "quat_scalar")
            continue
        full = n >= 4 and aligned[k]
        if full and (k in ("xyz", "scaling", "opacity") or (k == "f_dc" and M == 1)):
            br.add("vec16:" + k)
        elif full:
            br.add("sh_unstaged:" + k)
        if n % 4 or not aligned[k]:
            br.add("step_elem:" + k)
            if n >= 4 and not aligned[k]:
                br.add("step_elem_full:" + k)
    return br


def _adam_branches(quads, numels):
    br = set()
    for q, n in zip(quads, numels):
        if n >= 4 and _al(*q):
            br.add("vec16")
        if n % 4 or (n and not _al(*q)):
            br.add("scalar")
    return br


# ---- cases and checks ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _case(P, M, step, eps, seed=1):
    case = R.make_case(P, M, seed=seed, step=step)
    hyper = dict(step=step, eps=eps)
    r64, r32 = R.model_step_ref(case, torch.float64, **hyper), R.model_step_ref(case, torch.float32, **hyper)
    ok = R.judgeable(case, r64, **hyper)
    dropped = R.dropped_fraction(ok)
    assert dropped <= R.DROP_CAP, "%.3g of the elements cannot be judged" % dropped
    return dict(case=case, r64=r64, r32=r32, ok=ok, dropped=dropped, bar=R.bars(case, r64, r32, **hyper), hyper=hyper)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(c, got, what, **info):
    """Holds what one route returned against float64 at the derived bars; prints every figure first."""
    res = R.worst_ratios(got, c["r64"], c["bar"], c["ok"])
    print(json.dumps(dict(what=what, P=c["case"]["P"], M=c["case"]["M"], dropped=c["dropped"], **c["hyper"], **info,
                          worst_over_bar={k: float("%.4g" % v[3]) for k, v in res.items()},
                          figures={k: ["%.3g" % x for x in v[:3]] for k, v in res.items()})))
    for k, v in res.items():
        assert v[3] <= 1.0, "%s %s: err %.3g, e_ref %.3g, bar %.3g: %.3g of the bar" % (what, k, v[0], v[1], v[2], v[3])
    return res


def _check_untouched_elements(c, p_new, m_new, v_new, what):
    """g == 0, m == 0, v == 0: the element keeps p, m, v bit for bit (a quaternion: the whole row)."""
    case = c["case"]
    ups = case["ups"]
    zero_g = dict(xyz=ups["xyz"] == 0, f_dc=ups["shs"][:, :1] == 0, f_rest=ups["shs"][:, 1:] == 0, scaling=ups["scales"] == 0,
                  rotation=(ups["rotations"] == 0).all(1, keepdim=True).expand(-1, 4), opacity=ups["opacities"] == 0)
    seen = 0
    for k in R.GROUPS:
        still = zero_g[k] & (case["m"][k] == 0) & (case["v"][k] == 0)
        if k == "rotation":
            still = still.all(1, keepdim=True).expand(-1, 4)
        seen += int(still.sum())
        for new, old, name in ((p_new[k], case["p"][k], "p"), (m_new[k], case["m"][k], "m"), (v_new[k], case["v"][k], "v")):
            assert torch.equal(_bits(new.cpu())[still], _bits(old)[still]), "%s: %s.%s moved without a gradient" % (what, name, k)
    return seen


def _upload(c, arena):
    case = c["case"]
    for k in R.GROUPS:
        arena.put("p." + k, case["p"][k])
        arena.put("m." + k, case["m"][k])
        arena.put("v." + k, case["v"][k])
    for k, t in case["ups"].items():
        arena.put("g." + k, t)


def _hyper_args(c, lrs=None):
    lrs = R.default_lrs() if lrs is None else lrs
    return ((C.c_float * len(lrs))(*lrs), R.BETAS[0], R.BETAS[1], c["hyper"]["eps"], c["hyper"]["step"],
            C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _collect(c, arena, with_next):
    case = c["case"]
    p = {k: arena.t["p." + k].clone() for k in R.GROUPS}
    got = dict(m={k: arena.t["m." + k].clone() for k in R.GROUPS}, v={k: arena.t["v." + k].clone() for k in R.GROUPS},
               update={k: p[k].double().cpu() - case["p"][k].double() for k in R.GROUPS})
    if with_next:
        got["next"] = {k: arena.t["o." + k].clone() for k in R.ACTS}
    return p, got


def run_model_step(c, mode, outs, dev):
    """gsr_model_step through the C ABI on guarded views.  Returns (new parameters, got, branches)."""
    case = c["case"]
    P, M = case["P"], case["M"]
    arena = Arena(dev, offsets(mode))
    _upload(c, arena)
    if outs:
        for k, shape in (("scales", (P, 3)), ("rotations", (P, 4)), ("opacities", (P, 1)), ("shs", (P, M, 3))):
            arena.put("o." + k, shape=shape)
    VP = C.c_void_p * 6
    arr = lambda pre: VP(*[arena.ptr(pre + k) for k in R.GROUPS])  # noqa: E731
    o = (lambda k: C.c_void_p(arena.ptr("o." + k))) if outs else (lambda k: None)
    code = G.lib().gsr_model_step(P, M, arr("p."), arr("m."), arr("v."), *[C.c_void_p(arena.ptr("g." + k)) for k in
                                  ("xyz", "scales", "rotations", "opacities", "shs")], o("scales"), o("rotations"),
                                  o("opacities"), o("shs"), *_hyper_args(c))
    assert code >= 0, G.lib().gsr_last_error().decode()
    torch.cuda.synchronize()
    assert arena.guards_intact() is None, "guard floats of %s overwritten" % arena.guards_intact()
    for k, t in case["ups"].items():   # the one-kernel tail consumes the gradients without writing them
        assert torch.equal(_bits(arena.t["g." + k].cpu()), _bits(t))
    p, got = _collect(c, arena, outs)
    if outs:   # shs_out IS the updated leaves
        assert torch.equal(_bits(got["next"]["shs"]), _bits(torch.cat([p["f_dc"], p["f_rest"]], 1)))
    return p, got, _model_step_branches(P, M, arena.ptr, outs)


def run_three_kernels(c, mode, dev, zero_grads=1):
    """gsr_activate -> gsr_activate_backward -> gsr_adam_step (-> gsr_activate of the updated parameters) through the C
    ABI on guarded views.  Returns (new parameters, got, branches of k_adam / k_sh_move)."""
    case = c["case"]
    P, M = case["P"], case["M"]
    L = G.lib()
    arena = Arena(dev, offsets(mode))
    _upload(c, arena)
    shapes = dict(scales=(P, 3), rotations=(P, 4), opacities=(P, 1), shs=(P, M, 3))
    for pre in ("a.", "o."):
        for k in R.ACTS:
            arena.put(pre + k, shape=shapes[k])
    for k in ("scaling", "rotation", "opacity", "f_dc", "f_rest"):
        arena.put("r." + k, shape=case["p"][k].shape)
    vp = lambda name: C.c_void_p(arena.ptr(name))  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def activate(pre):
        return L.gsr_activate(P, M, vp("p.scaling"), vp("p.rotation"), vp("p.opacity"), vp("p.f_dc"), vp("p.f_rest"),
                              vp(pre + "scales"), vp(pre + "rotations"), vp(pre + "opacities"), vp(pre + "shs"), stream)

    assert activate("a.") >= 0, L.gsr_last_error().decode()
    assert L.gsr_activate_backward(P, M, vp("p.rotation"), vp("a.scales"), vp("a.opacities"), vp("g.scales"),
                                   vp("g.rotations"), vp("g.opacities"), vp("g.shs"), vp("r.scaling"), vp("r.rotation"),
                                   vp("r.opacity"), vp("r.f_dc"), vp("r.f_rest"), stream) >= 0, L.gsr_last_error().decode()
    torch.cuda.synchronize()
    gname = dict(xyz="g.xyz", f_dc="r.f_dc", f_rest="r.f_rest", scaling="r.scaling", rotation="r.rotation", opacity="r.opacity")
    got = dict(act={k: arena.t["a." + k].clone() for k in R.ACTS}, g={k: arena.t[gname[k]].clone() for k in R.GROUPS})
    # k_sh_move both ways (M > 1) and the M == 1 copies inside k_activate / k_activate_backward: bit for bit
    assert torch.equal(_bits(got["act"]["shs"].cpu()), _bits(torch.cat([case["p"]["f_dc"], case["p"]["f_rest"]], 1)))
    assert torch.equal(_bits(got["g"]["f_dc"].cpu()), _bits(case["ups"]["shs"][:, :1]))
    assert torch.equal(_bits(got["g"]["f_rest"].cpu()), _bits(case["ups"]["shs"][:, 1:]))
    VP = C.c_void_p * 6
    numels = [int(case["p"][k].numel()) for k in R.GROUPS]
    quads = [(arena.ptr("p." + k), arena.ptr(gname[k]), arena.ptr("m." + k), arena.ptr("v." + k)) for k in R.GROUPS]
    code = L.gsr_adam_step(6, VP(*[q[0] for q in quads]), VP(*[q[1] for q in quads]), VP(*[q[2] for q in quads]),
                           VP(*[q[3] for q in quads]), (C.c_size_t * 6)(*numels), *_hyper_args(c)[:5], int(zero_grads),
                           stream)
    assert code >= 0, L.gsr_last_error().decode()
    torch.cuda.synchronize()
    for k in R.GROUPS:   # zero_grads zeroes exactly the consumed gradients; 0 leaves them
        after = arena.t[gname[k]]
        if zero_grads:
            assert not bool(_bits(after).any()), k
        else:
            assert torch.equal(_bits(after), _bits(got["g"][k])), k
    assert activate("o.") >= 0, L.gsr_last_error().decode()
    torch.cuda.synchronize()
    assert arena.guards_intact() is None, "guard floats of %s overwritten" % arena.guards_intact()
    p, rest = _collect(c, arena, True)
    got.update(rest)
    br = {"adam:" + b for b in _adam_branches(quads, numels)}
    if M > 1:
        br.add("sh_move16" if _al(arena.ptr("a.shs")) else "sh_move_scalar")
        br.add("sh_split16" if _al(arena.ptr("g.shs")) else "sh_split_scalar")
    return p, got, br


def _same_bits(a, b):
    return {q + "." + k: bool(torch.equal(_bits(a[q][k]), _bits(b[q][k]))) for q in a if q in b for k in a[q]}


MODES = ("a0", "a4", "a8", "a12", "mix") + tuple("only:" + k for k in R.GROUPS)


@pytest.mark.parametrize("M,P", GRID)
def test_model_step_every_alignment(M, P, gpu_device):
    """gsr_model_step (k_model_step + k_sh_step) at every size seam, all tensors at 0 / 4 / 8 / 12 bytes and one group at
    a time.  Each mode names the branch it is there for; the restated launch conditions assert that it is selected."""
    step, eps = R.grid_hyper(GRID.index((M, P)))
    c = _case(P, M, step, eps)
    seen = set()
    for mode in MODES:
        if mode == "only:f_rest" and M == 1:
            continue
        p, got, br = run_model_step(c, mode, True, gpu_device)
        seen |= br
        if mode == "a0":       # everything aligned: 16-byte paths, aligned quaternions, SH leaves through LDS
            assert "quat16" in br and (M == 1 or "k_sh_step" in br) and (P < 2 or "vec16:xyz" in br)
            assert M > 1 or P < 2 or "vec16:f_dc" in br
        if mode in ("a4", "a8", "a12", "mix"):   # nothing aligned: step_elem for full groups, scalar quaternions
            assert "quat_scalar" in br and "k_sh_step" not in br and (P < 2 or "step_elem_full:xyz" in br)
        if mode == "only:rotation":
            assert "quat_scalar" in br and (M == 1 or "k_sh_step" in br)
        if mode == "only:f_dc" and M > 1:   # f_dc group misaligned, f_rest aligned: SH leaf without LDS staging
            assert "k_sh_step" not in br and "step_elem:f_dc" in br
            assert 3 * (M - 1) * P < 4 or "sh_unstaged:f_rest" in br
        if mode == "only:f_rest":           # the reverse
            assert "k_sh_step" not in br and "step_elem:f_rest" in br and (P < 2 or "sh_unstaged:f_dc" in br)
        _check(c, got, "model_step", mode=mode, branches=sorted(br))
        _check_untouched_elements(c, p, got["m"], got["v"], "model_step " + mode)
        if mode in ("a0", "a8"):
            p2, again, _ = run_model_step(c, mode, True, gpu_device)   # two runs are bitwise equal
            assert all(_same_bits(got, again).values()) and all(torch.equal(_bits(p[k]), _bits(p2[k])) for k in p)
            p3, bare, br3 = run_model_step(c, mode, False, gpu_device)  # all four *_out null: same parameters and moments
            assert all(torch.equal(_bits(p[k]), _bits(p3[k])) for k in p) and all(_same_bits(bare, got).values())
            # "same arithmetic" as the three kernels (k_model_step's header): reported, not asserted -- both are held
            # to float64 at the same bars, and the compiler may contract a multiply-add in one kernel and not the other
            same = _same_bits(got, run_three_kernels(c, mode, gpu_device)[1])
            print(json.dumps(dict(what="one kernel vs three, bitwise", P=P, M=M, mode=mode,
                                  differs=sorted(k for k, v in same.items() if not v))))
    if P >= 4:
        assert {"vec16:xyz", "vec16:scaling", "vec16:opacity", "step_elem_full:xyz", "quat16", "quat_scalar"} <= seen
    if P >= 4 and M > 1:
        assert {"k_sh_step", "sh_unstaged:f_rest", "sh_unstaged:f_dc", "step_elem_full:f_dc", "step_elem_full:f_rest"} <= seen


@pytest.mark.parametrize("M,P", GRID)
def test_three_kernels_every_alignment(M, P, gpu_device):
    """gsr_activate / gsr_activate_backward / gsr_adam_step (k_activate, k_sh_move both ways, k_activate_backward, k_adam)
    on the same grid, each held to float64."""
    step, eps = R.grid_hyper(GRID.index((M, P)))
    c = _case(P, M, step, eps)
    seen = set()
    for i, mode in enumerate(("a0", "a4", "a8", "a12", "mix")):
        p, got, br = run_three_kernels(c, mode, gpu_device, zero_grads=i % 2 == 0)
        seen |= br
        if mode == "a0":
            assert (P < 2 or "adam:vec16" in br) and (M == 1 or {"sh_move16", "sh_split16"} <= br)
        elif mode != "mix":
            assert "adam:scalar" in br and "adam:vec16" not in br and (M == 1 or {"sh_move_scalar", "sh_split_scalar"} <= br)
        _check(c, got, "three_kernels", mode=mode, branches=sorted(br))
        _check_untouched_elements(c, p, got["m"], got["v"], "three_kernels " + mode)
        if mode in ("a0", "a8"):
            p2, again, _ = run_three_kernels(c, mode, gpu_device, zero_grads=i % 2 == 0)
            assert all(_same_bits(got, again).values()) and all(torch.equal(_bits(p[k]), _bits(p2[k])) for k in p)


@pytest.mark.parametrize("mode", ["a0", "a8"])
def test_large_model(mode, gpu_device):
    """P = 200 003 (one case: the references run on the CPU) at M = 4: many workgroups of every kernel, odd tails."""
    c = _case(P_LARGE, 4, 10, 1e-15)
    p, got, br = run_model_step(c, mode, True, gpu_device)
    assert ("k_sh_step" in br) == (mode == "a0")
    _check(c, got, "model_step large", mode=mode, branches=sorted(br))
    _check_untouched_elements(c, p, got["m"], got["v"], "large " + mode)
    p, got, br = run_three_kernels(c, mode, gpu_device)
    _check(c, got, "three_kernels large", mode=mode, branches=sorted(br))


@pytest.mark.parametrize("eps", R.EPSES)
@pytest.mark.parametrize("step", R.STEPS)
@pytest.mark.parametrize("M", [1, 4])
def test_every_step_count_and_eps(M, step, eps, gpu_device):
    """Steps 1 ... 30 000 (bias corrections from 0.1 / 0.001 to 1) x both eps, on both routes, aligned and not."""
    c = _case(257, M, step, eps, seed=2)
    for mode in ("a0", "a12"):
        p, got, br = run_model_step(c, mode, True, gpu_device)
        _check(c, got, "model_step", mode=mode)
        n = _check_untouched_elements(c, p, got["m"], got["v"], "model_step")
        assert n > 0
        p, got, br = run_three_kernels(c, mode, gpu_device)
        _check(c, got, "three_kernels", mode=mode)
        assert _check_untouched_elements(c, p, got["m"], got["v"], "three_kernels") == n


def test_updated_quaternion_is_what_gets_normalised(gpu_device):
    """Unit quaternions and a large rotation learning rate: rotations_out must be normalize(q_new), far from
    normalize(q_old) (checked: the two differ by more than 100 bars somewhere)."""
    case = R.make_case(129, 1, seed=4, step=1, quats="unit")
    lrs = R.default_lrs()
    lrs[4] = float(torch.tensor(0.25, dtype=torch.float32))
    hyper = dict(step=1, eps=1e-15, lrs=lrs)
    r64, r32 = R.model_step_ref(case, torch.float64, **hyper), R.model_step_ref(case, torch.float32, **hyper)
    ok = R.judgeable(case, r64, **hyper)
    c = dict(case=case, r64=r64, r32=r32, ok=ok, dropped=R.dropped_fraction(ok), bar=R.bars(case, r64, r32, **hyper),
             hyper=dict(step=1, eps=1e-15))
    assert float(((r64["next"]["rotations"] - r64["act"]["rotations"]).abs() / c["bar"]["next"]["rotations"][1]).max()) > 100
    arena = Arena(gpu_device, offsets("a0"))
    _upload(c, arena)
    for k, shape in (("scales", (129, 3)), ("rotations", (129, 4)), ("opacities", (129, 1)), ("shs", (129, 1, 3))):
        arena.put("o." + k, shape=shape)
    VP = C.c_void_p * 6
    arr = lambda pre: VP(*[arena.ptr(pre + k) for k in R.GROUPS])  # noqa: E731
    assert G.lib().gsr_model_step(129, 1, arr("p."), arr("m."), arr("v."), *[C.c_void_p(arena.ptr("g." + k)) for k in
                                  ("xyz", "scales", "rotations", "opacities", "shs")], *[C.c_void_p(arena.ptr("o." + k))
                                  for k in R.ACTS], *_hyper_args(c, lrs)) >= 0
    torch.cuda.synchronize()
    _, got = _collect(c, arena, True)
    _check(c, got, "model_step lr_rotation=0.25")


# sizes = 0 ... 3 mod 4 and empty tensors: (P, M, group) -> numel 3P / 3P / 3(M-1)P
ADAM_SETS = {1: [(3, 2, "f_rest")],
             6: [(1, 1, "xyz"), (1, 1, "f_rest"), (2, 2, "f_dc"), (3, 2, "f_rest"), (4, 4, "xyz"), (63, 4, "f_rest")],
             8: [(257, 1, "xyz"), (2, 1, "f_rest"), (1, 2, "f_rest"), (2, 4, "f_rest"), (3, 1, "f_dc"), (64, 2, "f_dc"),
                 (5, 1, "f_rest"), (129, 9, "f_rest")]}


@pytest.mark.parametrize("mode", ["a0", "a4", "a8", "a12", "mix"])
@pytest.mark.parametrize("zero_grads", [0, 1])
@pytest.mark.parametrize("n", [1, 6, 8])
def test_adam_step_tensor_counts(n, zero_grads, mode, gpu_device):
    """gsr_adam_step with 1, 6 and 8 tensors, some empty, numel = 0 ... 3 mod 4, each with its own learning rate.  The
    tensors are identity-activation groups of small cases, so the float64 Adam of optim_ref applies unchanged."""
    step, eps = 10, 1e-8
    lr_of = dict(zip(R.GROUPS, R.default_lrs()))
    arena = Arena(gpu_device, offsets(mode))
    items = []
    for i, (P, M, grp) in enumerate(ADAM_SETS[n]):
        c = _case(P, M, step, eps, seed=7)
        case = c["case"]
        g = dict(xyz=case["ups"]["xyz"], f_dc=case["ups"]["shs"][:, :1], f_rest=case["ups"]["shs"][:, 1:])[grp].contiguous()
        for pre, src in (("p", case["p"][grp]), ("g", g), ("m", case["m"][grp]), ("v", case["v"][grp])):
            arena.put("%s.%d" % (pre, i), src)
        items.append((c, grp, g))
    assert sorted({int(it[2].numel()) % 4 for it in items if it[2].numel()}) == ([1] if n == 1 else [0, 1, 2, 3])
    assert n == 1 or any(it[2].numel() == 0 for it in items)
    VP = C.c_void_p * n
    arr = lambda pre: VP(*[arena.ptr("%s.%d" % (pre, i)) for i in range(n)])  # noqa: E731
    numels = [int(it[2].numel()) for it in items]
    code = G.lib().gsr_adam_step(n, arr("p"), arr("g"), arr("m"), arr("v"), (C.c_size_t * n)(*numels),
                                 (C.c_float * n)(*[lr_of[it[1]] for it in items]), R.BETAS[0], R.BETAS[1], eps, step,
                                 zero_grads, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code >= 0, G.lib().gsr_last_error().decode()
    torch.cuda.synchronize()
    assert arena.guards_intact() is None
    br = _adam_branches([tuple(arena.ptr("%s.%d" % (pre, i)) for pre in "pgmv") for i in range(n)], numels)
    assert "scalar" in br and (("vec16" in br) == (mode == "a0"))   # "mix": p / g / m / v of a tensor at 0 / 4 / 8 / 12
    for i, (c, grp, g) in enumerate(items):
        if not g.numel():
            continue
        after = arena.t["g.%d" % i].cpu()
        assert (not bool(_bits(after).any())) if zero_grads else torch.equal(_bits(after), _bits(g))
        p = arena.t["p.%d" % i]
        got = dict(m={grp: arena.t["m.%d" % i]}, v={grp: arena.t["v.%d" % i]},
                   update={grp: p.double().cpu() - c["case"]["p"][grp].double()})
        _check(c, got, "adam_step", n=n, tensor=i, mode=mode, branches=sorted(br))


def _python_model(c, dev, growable):
    case = c["case"]
    P, M = case["P"], case["M"]
    names = dict(_xyz="xyz", _features_dc="f_dc", _features_rest="f_rest", _scaling="scaling", _rotation="rotation",
                 _opacity="opacity")
    if not growable:
        m = G.GaussianParameters(*[case["p"][k].to(dev) for k in R.GROUPS])
        return m, names, None
    m = G.GrowableGaussians(600, M, dev)   # three growths to P = 1025; the second crosses the capacity, which doubles
    opt = G.GrowableAdam(m, eps=c["hyper"]["eps"])
    gen = torch.Generator().manual_seed(0)
    for n in (341, 342, P - 683):
        a = torch.randn(n, 3, 3, generator=gen)
        m.add_new_pointcloud(torch.randn(n, 3, generator=gen).to(dev), (a @ a.transpose(1, 2)).to(dev),
                             (torch.rand(n, 3, generator=gen) * 255).to(dev))
    assert m.P == P and m.capacity == 1200
    with torch.no_grad():
        for attr, k in names.items():
            getattr(m, attr).copy_(case["p"][k].to(dev))
            mm, vv = m.moments(attr)
            mm.copy_(case["m"][k].to(dev))
            vv.copy_(case["v"][k].to(dev))
            assert getattr(m, attr).data_ptr() == m._buf[attr].data_ptr()   # leaves are views of the capacity buffers
    return m, names, opt


@pytest.mark.parametrize("growable", [False, True])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("M,step", [(1, 1), (4, 1), (4, 10), (9, 1000)])
def test_python_routes(M, step, tail, growable, gpu_device):
    """FusedActivations + FusedAdam.step, GaussianParameters.fused_tail + step_model, and both on a GrowableGaussians
    whose leaves and moments are views of capacity buffers after a growth that crossed the capacity."""
    dev = gpu_device
    c = _case(1025, M, step, 1e-15, seed=5)
    case = c["case"]
    m, names, opt = _python_model(c, dev, growable)
    m.fused_tail = tail
    if opt is None:
        opt = G.FusedAdam(m.param_groups(), eps=1e-15)
        for attr, k in names.items():
            if case["p"][k].numel():
                opt.state[getattr(m, attr)] = dict(exp_avg=case["m"][k].to(dev), exp_avg_sq=case["v"][k].to(dev))
    opt._step = step - 1
    xyz, op, sc, rot, shs = m.activated()
    got = dict(act=dict(scales=sc.detach().clone(), rotations=rot.detach().clone(), opacities=op.detach().clone(),
                        shs=shs.detach().clone()))
    ups = {k: t.to(dev) for k, t in case["ups"].items()}
    torch.autograd.backward([xyz, sc, rot, op, shs], [ups["xyz"], ups["scales"], ups["rotations"], ups["opacities"], ups["shs"]])
    if tail:
        opt.step_model(m)
        got["next"] = dict(zip(R.ACTS, m._next_act))
    else:
        got["g"] = {k: getattr(m, attr).grad.clone() for attr, k in names.items() if case["p"][k].numel()}
        opt.step()
        assert all(not bool(getattr(m, attr).grad.any()) for attr in names if getattr(m, attr).grad is not None)
    p = {k: getattr(m, attr).detach() for attr, k in names.items()}
    live = [k for k in R.GROUPS if case["p"][k].numel()]
    got["m"] = {k: opt.state[getattr(m, attr)]["exp_avg"] for attr, k in names.items() if k in live}
    got["v"] = {k: opt.state[getattr(m, attr)]["exp_avg_sq"] for attr, k in names.items() if k in live}
    got["update"] = {k: p[k].double().cpu() - case["p"][k].double() for k in live}
    _check(c, got, "python", tail=tail, growable=growable)
    _check_untouched_elements(c, p, {k: got["m"].get(k, case["m"][k]) for k in R.GROUPS},
                              {k: got["v"].get(k, case["v"][k]) for k in R.GROUPS}, "python")
    if growable:   # the rows beyond P of the capacity buffers stay the zeros they were created with
        for attr in names:
            for store in (m._buf, m._m, m._v):
                assert not bool(store[attr][m.P:].any())
