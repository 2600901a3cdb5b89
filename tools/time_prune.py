"""Times one prune of a 2 M-row model (GPU): gsr_prune_mark + gsr_prune_compact on the 18 tensors (six leaves and both
Adam moments) against the same operation done the reference's way in the same process -- the drop mask from Torch ops,
nonzero, and 18 index_select (GaussianModel::prune_optimizer, src/gs/gaussian.cu:430-449, per group) -- and
k_prune_compact on its own, whose achieved bytes/s (reads of P rows + writes of P' rows) stands beside k_model_step's
streaming rate on the same buffers.
    python tools/time_prune.py [--rows 2000000] [--iters 20] [--repeats 5] [--out profiles/prune_timing.json]
Device events around `iters` prunes, the routes alternating within every repeat; medians and min..max of the repeats."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2_000_000)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_timing.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
LO, HI = 1.0 / 255.0, 0.3


def model(P, M, share_dropped, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen).to(dev)  # noqa: E731
    shapes = ((3,), (1, 3), (M - 1, 3), (3,), (4,), (1,))
    leaves = [r(P, *s) for s in shapes]
    leaves[3] = leaves[3] * 0.3 - 3.0
    dead = torch.rand(P, generator=gen).to(dev) < share_dropped
    even = torch.arange(P, device=dev) % 2 == 0
    leaves[3][dead & even, 1] = 0.5
    leaves[5][dead & ~even] = -9.0
    return leaves + [r(P, *s) for s in shapes] + [r(P, *s).abs() for s in shapes]   # params, exp_avg, exp_avg_sq


def hip_route(t, dst):
    reasons, row_map, counts = _capi.prune_mark(t[0], t[3], t[4], t[5], LO, HI, True)
    _capi.prune_compact(t, dst, reasons, row_map)
    return reasons, row_map, counts


def torch_route(t):
    xyz, scaling, rot, opac = t[0], t[3], t[4], t[5]
    drop = (torch.sigmoid(opac).view(-1) < LO) | (torch.exp(scaling) > HI).any(1)
    drop |= ~(torch.isfinite(xyz).all(1) & torch.isfinite(scaling).all(1) & torch.isfinite(rot).all(1) &
              torch.isfinite(opac).all(1))
    idx = (~drop).nonzero().view(-1)
    return [x.index_select(0, idx) for x in t]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


rows = []
for M in (1, 16):
    for share in (0.03, 0.5):
        P = args.rows
        t = model(P, M, share, seed=M)
        reasons, row_map, counts = _capi.prune_mark(t[0], t[3], t[4], t[5], LO, HI, True)
        P_new = int(counts[0])
        dst = [torch.empty((P_new,) + tuple(x.shape[1:]), device=dev) for x in t]
        for _ in range(3):   # warm-up of every route
            hip_route(t, dst)
            ref = torch_route(t)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(dst, ref))
        del ref
        row_floats = sum(int(x[0].numel()) for x in t)
        nbytes = 4 * row_floats * (P + P_new)
        reps = []
        for rep in range(args.repeats):
            reps.append(dict(hip_us=timed(lambda: hip_route(t, dst), args.iters),
                             torch_us=timed(lambda: torch_route(t), args.iters),
                             mark_us=timed(lambda: _capi.prune_mark(t[0], t[3], t[4], t[5], LO, HI, True), args.iters),
                             compact_us=timed(lambda: _capi.prune_compact(t, dst, reasons, row_map), args.iters)))
        med = lambda k: round(statistics.median(x[k] for x in reps), 1)  # noqa: E731
        span = lambda k: [round(min(x[k] for x in reps), 1), round(max(x[k] for x in reps), 1)]  # noqa: E731
        row = dict(P=P, M=M, P_new=P_new, share_dropped=round(1 - P_new / P, 4), bit_identical_to_torch=same,
                   iters=args.iters, repeats=args.repeats, bytes_moved=nbytes,
                   **{k: dict(median=med(k), span=span(k)) for k in ("hip_us", "torch_us", "mark_us", "compact_us")},
                   compact_TB_per_s=round(nbytes / (med("compact_us") * 1e-6) / 1e12, 3),
                   speedup_over_torch=round(med("torch_us") / med("hip_us"), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del t, dst
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(rows, fh, indent=1)
    fh.write("\n")
