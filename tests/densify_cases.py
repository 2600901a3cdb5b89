"""The inputs of test_gpu_densify.py, kept here so that test_densify_ref.py can hold the float32 restatement to every bar
on the same inputs without a device.  numpy only; every generator is deterministic in its arguments."""
import numpy as np

import densify_ref as D

PAT = 0x7FC0DEAD                     # arena.PAT: a quiet NaN no kernel produces
ACC_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
GRAD_THRESHOLD = 2.0 ** -12          # a power of two: views * threshold is exact, so a row can sit ON the threshold
SIZE_THRESHOLD = 0.01
# every seam of the 256-row workgroups, and 1 027 workgroups: k_densify_scan takes 1 024 totals per pass, so the last size
# runs its loop twice -- a full pass, the carry, and a partial second pass of three totals
MARK_SIZES = (1, 255, 256, 257, 511, 512, 513, 1025, 262_144 + 600)
MARK_PATTERNS = ("none", "all", "alternating", "one_per_workgroup", "0.05", "0.5")
APPLY_CASES = ((1, 1), (257, 1), (300, 4), (700, 16))    # (P, M): one row; more than one workgroup; every SH width class


def accumulate_case(P, seed=0):
    """three views [(radii int32 [P], grad f32 [P,3])] and the initial stats: zero, except that the rows NO view touches
    carry the NaN pattern, which must come back bit for bit"""
    rng = np.random.default_rng(1000 * P + seed)
    views = []
    for v in range(3):
        radii = rng.integers(1, 60, P).astype(np.int32)
        kind = rng.integers(0, 3, P)                       # zero / positive / negative radii in every view
        radii[kind == 0] = 0
        radii[kind == 2] = -radii[kind == 2]
        mag = 10.0 ** rng.uniform(-20, 8, (P, 3))
        g = (mag * rng.choice([-1.0, 1.0], (P, 3))).astype(np.float32)
        special = rng.integers(0, 12, P)
        g[special == 0, 0] = 0.0
        g[special == 1] = 0.0                              # a visible row with a zero gradient still counts as a view
        g[special == 2, 0] = np.nan
        g[special == 3, 1] = np.inf
        g[special == 4, 0] = -np.inf
        g[special == 5, 2] = np.nan                        # the third column is not read
        g[special == 6] = np.float32(3e19)                 # finite components whose squares overflow: the norm is +Inf
        views.append((radii, g))
    touched = np.zeros(P, dtype=bool)
    for radii, g in views:
        touched |= D.accumulate(np.zeros((P, 3)), radii, g, np.float32)[:, 1] > 0
    stats0 = np.zeros((P, 3), dtype=np.float32)
    stats0.view(np.uint32)[~touched] = PAT
    return views, stats0, touched


def mark_case(P, pattern, seed=0):
    """(stats f32 [P,3], scaling_raw f32 [P,3], wanted candidate mask or None).  Candidates average 2 * threshold, the
    others threshold / 2; scales are log-uniform over [-12, 2]."""
    rng = np.random.default_rng(7 * P + seed)
    i = np.arange(P)
    if pattern == "none":
        cand = np.zeros(P, dtype=bool)
    elif pattern == "all":
        cand = np.ones(P, dtype=bool)
    elif pattern == "alternating":
        cand = i % 2 == 1
    elif pattern == "one_per_workgroup":
        cand = i % 256 == 37 % max(min(P, 256), 1)
    else:
        cand = rng.random(P) < float(pattern)
    views = rng.integers(1, 6, P).astype(np.float32)
    avg = np.where(cand, 2.0 * GRAD_THRESHOLD, 0.5 * GRAD_THRESHOLD) * rng.uniform(0.9, 1.1, P)
    stats = np.stack([(avg * views), views, rng.integers(0, 50, P)], 1).astype(np.float32)
    scaling = rng.uniform(-12.0, 2.0, (P, 3)).astype(np.float32)
    return stats, scaling, cand


def mark_boundary_case():
    """(stats, scaling, expected kinds): the rows the rule's wording decides.  size_threshold = 1.0 here."""
    T = np.float32(GRAD_THRESHOLD)
    below = np.nextafter(T, np.float32(0))
    rows = [  # grad_sum, views, scaling, kind
        (T * 3, 3, (-1, -2, -3), 1),                  # avg exactly ON the threshold: a candidate (>=)
        (below, 1, (-1, -2, -3), 0),                  # one float below it
        (1e9, 0, (-1, -2, -3), 0),                    # views = 0: avg = 0
        (1e9, -1, (-1, -2, -3), 0),                   # (views never goes negative; the rule still says views > 0)
        (np.nan, 2, (-1, -2, -3), 0),                 # a NaN compares false
        (1.0, np.nan, (-1, -2, -3), 0),
        (np.inf, 2, (-1, -2, -3), 1),                 # +Inf >= threshold
        (1.0, 1, (0, -2, -3), 1),                     # exp(0) = 1 against size_threshold 1: strict, so NOT big
        (1.0, 1, (-2, 0, 0), 1),
        (1.0, 1, (-2, -3, 1e-3), 2),                  # just big, in the last component
        (1.0, 1, (0.5, -3, -3), 2),
        (1.0, 1, (np.nan, -3, -3), 0),                # non-finite scaling: no candidate, whatever the gradient
        (1.0, 1, (-3, np.inf, -3), 0),
        (1.0, 1, (-3, -3, -np.inf), 0),
        (1.0, 1, (-3, -3, -80), 1),                   # a finite scale that underflows is simply small
    ]
    stats = np.array([[r[0], r[1], 5] for r in rows], dtype=np.float32)
    scaling = np.array([r[2] for r in rows], dtype=np.float32)
    return stats, scaling, np.array([r[3] for r in rows], dtype=np.uint8)


def apply_case(P, M, seed=0, marked=0.4):
    """leaves (six f32 arrays), moments (twelve: exp_avg then exp_avg_sq), stats, kinds, offsets.  Quaternions: unit,
    scaled by 1e-6 ... 1e4, and zero (the clamp); scaling_raw over [-12, 2]; about `marked` of the rows marked, half of
    them split, with the first and the last row marked when P allows."""
    rng = np.random.default_rng(31 * P + M + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    q = rng.standard_normal((P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cls = rng.integers(0, 4, P)
    q[cls == 1] *= 10.0 ** rng.uniform(-6, 4, (int((cls == 1).sum()), 1))
    q[cls == 2] = 0.0
    leaves = [f(P, 3) * 10, f(P, 1, 3), f(P, M - 1, 3) * np.float32(0.1), rng.uniform(-12, 2, (P, 3)).astype(np.float32),
              q.astype(np.float32), f(P, 1)]
    moments = [f(*a.shape) for a in leaves] + [np.abs(f(*a.shape)) for a in leaves]
    stats = np.abs(f(P, 3)) + np.float32(1)
    kinds = np.where(rng.random(P) < marked, rng.integers(1, 3, P), 0).astype(np.uint8)
    kinds[0] = 2
    kinds[-1] = 1 if P > 1 else 2
    offsets = np.concatenate([[0], np.cumsum(kinds != 0)]).astype(np.int32)
    return leaves, moments, stats, kinds, offsets
