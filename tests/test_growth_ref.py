"""CPU anchor of tests/growth_ref.py, the float64 reference k_init_gaussians is held to (test_gpu_growth_ref64.py)."""
import json
import math

import pytest
import torch

import growth_ref as R


def test_restatement_on_values_known_by_hand():
    covs = torch.zeros(4, 3, 3)
    covs[0].diagonal().copy_(torch.tensor([2.0, 8.0, 0.5]))           # * 0.5 -> 1, 4, 0.25
    covs[1].diagonal().copy_(torch.tensor([0.0, -1.0, 3e38]))          # -> -inf, NaN, finite (1.5e38)
    covs[2].diagonal().copy_(torch.tensor([-0.0, 1e-40, 2.0 * math.e ** 2]))
    covs[3] = float("nan")
    covs[3].diagonal().copy_(torch.tensor([2.0, 2.0, 2.0]))            # NaN off the diagonal is never read
    rgbs = torch.tensor([[0.0, 255.0, 127.5]] * 4)
    for dt in (torch.float64, torch.float32):
        s, f = R.init_ref(covs, rgbs, 0.5, dt)
        assert s[0].tolist() == [0.0, pytest.approx(math.log(2.0), rel=1e-7), pytest.approx(math.log(0.5), rel=1e-7)]
        assert s[1, 0] == -math.inf and math.isnan(s[1, 1]) and math.isfinite(s[1, 2])
        assert s[2, 0] == -math.inf and math.isfinite(s[2, 1]) and float(s[2, 2]) == pytest.approx(1.0, abs=1e-6)
        assert s[3].tolist() == [0.0, 0.0, 0.0]
        assert f[0].tolist() == [pytest.approx(-0.5 / R.C0, rel=1e-6), pytest.approx(0.5 / R.C0, rel=1e-6), 0.0]
    assert R.ieee_class(torch.tensor([1.0, math.inf, -math.inf, math.nan])).tolist() == [0, 1, 2, 3]
    s32, _ = R.init_ref(torch.full((1, 3, 3), 3e38), rgbs[:1], 4.0, torch.float32)   # overflows in float32 only
    s64, _ = R.init_ref(torch.full((1, 3, 3), 3e38), rgbs[:1], 4.0, torch.float64)
    assert bool(torch.isposinf(s32).all()) and bool(torch.isfinite(s64).all())


@pytest.mark.parametrize("scale", R.SCALES)
def test_float32_restatement_stays_inside_the_floors(scale):
    worst = {}
    for n in R.NS:
        xyz, covs, rgbs = R.cloud(n, 1, scale)
        s32, f32 = R.init_ref(covs, rgbs, scale, torch.float32)
        fs, ff = R.floors(covs, rgbs, scale)
        res = R.judge(s32, f32, covs, rgbs, scale)      # classes against itself; ratio against max(2 e_ref, floor)
        s64, f64 = R.init_ref(covs, rgbs, scale, torch.float64)
        ok = torch.isfinite(s32) & torch.isfinite(s64)
        rs = float(((s32 - s64).abs()[ok] / fs[ok]).max())
        rf = float(((f32 - f64).abs() / ff.clamp(min=1e-300)).max())
        assert rs <= 1.0 and rf <= 1.0, (n, rs, rf)
        worst[n] = (round(rs, 3), round(rf, 3))
        assert all(v[2] <= 0.5 + 1e-12 for v in res.values())
        if n >= 255:   # the generator reaches every class and a product of exactly 1
            cls = R.ieee_class(s32)
            assert bool((cls == 2).any()) and bool((cls == 3).any()) and bool((s32 == 0).any())
            assert scale <= 1 or bool((cls == 1).any())
            assert bool(torch.isnan(xyz).any()) and bool((R.bits(xyz) == -2 ** 31).any())
    print(json.dumps(dict(what="float32 init restatement over floor (scaling, f_dc)", scale=scale, worst=worst)))
