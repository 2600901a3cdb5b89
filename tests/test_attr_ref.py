"""CPU tests of the attribute-blend reference itself (tests/attr_ref.py): before the HIP kernel is held to it, the
reference is held to the oracle's silhouette and to the conditions the GPU comparison relies on."""
import functools

import numpy as np
import pytest

import attr_ref as AR
import contrib_ref as CR
from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def _frame(cfg):
    return O.forward(CR.scene(*cfg))


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_fragile_share_stays_below_the_cap(cfg):
    share = float((_frame(cfg).fragile != 0).mean())
    print("fragile share %.2e" % share)
    assert share <= AR.MAX_FRAGILE_SHARE


@pytest.mark.parametrize("cfg", CR.SCENES)
def test_unit_attribute_equals_the_oracle_silhouette(cfg):
    fr = _frame(cfg)
    out, scale = AR.blend64(fr, np.ones((fr.P, 1)))
    ok = fr.fragile == 0
    assert np.array_equal(out, scale) and (out >= 0).all()
    d = np.abs(out[0] - fr.out_acc[0].astype(np.float64))[ok]
    print("worst |walk64 - out_acc| %.3e" % d.max())
    assert fr.out_acc.max() > 0.5 and d.max() <= 1e-4          # the oracle's image bar (BASELINE.json north_star)
    # a pixel nothing was blended into reads exactly zero
    assert not out[0][fr.n_contrib == 0].any()


def test_float32_yardstick_stays_within_the_recorded_ratio():
    worst = 0.0
    for cfg in CR.SCENES:
        fr = _frame(cfg)
        ok = fr.fragile == 0
        for C in (1, 2, 3, 4):
            at = AR.attributes(fr.P, C)
            out, scale = AR.blend64(fr, at)
            worst = max(worst, AR.worst_ratio(AR.yardstick32(fr, at), out, scale, ok))
    print("yardstick32 worst |d| / sum w |attr|: %.3e" % worst)
    # AR.YARDSTICK is what the GPU bar is 8 x of: it must be what the reference measures, not a number from elsewhere
    assert 0.5 * AR.YARDSTICK <= worst <= AR.YARDSTICK


def test_channels_are_blended_independently():
    fr = _frame(CR.SCENES[0])
    at = AR.attributes(fr.P, 3)
    out3, _ = AR.blend64(fr, at)
    for c in range(3):
        np.testing.assert_allclose(AR.blend64(fr, at[:, c:c + 1])[0][0], out3[c], rtol=1e-12, atol=1e-15)
