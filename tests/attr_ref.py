"""Reference of the attribute blend (gsr_blend_attributes): CPU, numpy, test infrastructure only.

blend64(fr, attr) walks every tile's list of an oracle frame (oracle.oracle.forward) with contrib_ref._tile_walk -- the
CUTS decided in float32 on the frame's own 2-D values, `index < n_contrib[pixel]` as the termination -- and carries the
weights alpha * T and the sums  sum_i w_i attr[i][c]  in float64.  It also returns  sum_i w_i |attr[i][c]|, the scale
the comparison is relative to (a signed attribute cancels; the error of a float32 sum does not shrink with its value).

yardstick32(fr, attr) takes the same walk in float32 throughout, in the forward's order: T <- T * (1 - alpha), w = alpha * T,
acc <- fma(attr, w, acc) entry by entry.

A pixel the oracle flags `fragile` may legitimately decide a cut differently in another float32 implementation: it is
excluded from every comparison.  The excluded share is capped at MAX_FRAGILE_SHARE per scene (measured on
contrib_ref.SCENES: 0, 0 and 3.0e-5; tests/test_attr_ref.py asserts the cap).

Bar.  worst |yardstick32 - float64| / sum w |attr| over contrib_ref.SCENES with the attributes of `attributes()`,
channels 1..4, measured on the CPU: 2.57e-6 (tests/test_attr_ref.py holds the reference to it).  The GPU comparison
allows B = 8 x 2.6e-6 = 2.08e-5: the margin covers the hardware exp2, the pre-scaled conic and a different summation
tree (contrib_ref.B's convention).
"""
import numpy as np

import contrib_ref as CR

F32 = np.float32
MAX_FRAGILE_SHARE = 0.01
YARDSTICK = 2.6e-6
B = 8.0 * YARDSTICK


def attributes(P, C, seed=5):
    """[P, C] float32, signed, of order one"""
    return np.random.default_rng(seed).normal(0.0, 1.0, (P, C)).astype(F32)


def _weights64(take, dx, dy, co):
    dx, dy, co = dx.astype(np.float64), dy.astype(np.float64), co.astype(np.float64)
    power = -0.5 * (co[None, :, 0] * dx * dx + co[None, :, 2] * dy * dy) - co[None, :, 1] * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.where(take, np.minimum(0.99, co[None, :, 3] * np.exp(power)), 0.0)
    T = np.cumprod(np.concatenate([np.ones_like(a[:, :1]), 1.0 - a[:, :-1]], 1), 1)
    return a * T


def blend64(fr, attr):
    """(out64 [C,H,W], scale64 [C,H,W] = sum w |attr|), float64"""
    attr = np.asarray(attr, np.float64).reshape(fr.P, -1)
    C = attr.shape[1]
    out, scale = np.zeros((C, fr.H, fr.W)), np.zeros((C, fr.H, fr.W))
    for t in range(fr.ranges.shape[0]):
        ids, ys, xs, take, _, (dx, dy, co) = CR._tile_walk(fr, t)
        if len(ids) == 0:
            continue
        w = _weights64(take, dx, dy, co)
        out[:, ys, xs] = (w @ attr[ids]).T
        scale[:, ys, xs] = (w @ np.abs(attr[ids])).T
    return out, scale


def yardstick32(fr, attr):
    """out32 [C,H,W] float32: the walk in float32 throughout, in the forward's order"""
    attr = np.asarray(attr, F32).reshape(fr.P, -1)
    C = attr.shape[1]
    out = np.zeros((C, fr.H, fr.W), F32)
    for t in range(fr.ranges.shape[0]):
        ids, ys, xs, take, alpha, _ = CR._tile_walk(fr, t)
        if len(ids) == 0:
            continue
        a = np.where(take, alpha, F32(0))
        T = np.cumprod(np.concatenate([np.ones_like(a[:, :1]), F32(1) - a[:, :-1]], 1), 1, dtype=F32)
        w = (a * T).astype(F32)
        acc = np.zeros((len(ys), C), F32)
        for j in range(len(ids)):   # fma(attr, w, acc): the product of two float32 is exact in float64
            acc = (acc.astype(np.float64) + w[:, j, None].astype(np.float64) * attr[ids[j]][None, :].astype(np.float64)).astype(F32)
        out[:, ys, xs] = acc.T
    return out


def worst_ratio(got, ref, scale, ok):
    """max |got - ref| / scale over the pixels of `ok` with scale > 0 (all channels)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = (scale > 0) & ok[None]
    return float((np.abs(got - ref)[m] / scale[m]).max(initial=0.0))
