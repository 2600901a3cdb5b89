"""Times the per-Gaussian blend contribution pass (gsr_contribution + gsr_contribution_finish) beside the forward blend
it re-walks and beside the only other route to the weight sum: a whole gsr_backward with unit upstream.

    python tools/time_contribution.py [--iters 30] [--warmup 5] [--out FILE.jsonl]

Shapes: BASELINE C3 (2 M Gaussians, 1920x1080) and the product shape (300 k Gaussians, 640x512), with precomputed
colours (the backward route reads dL_dcolors).  One forward per shape (synchronous, then the product's speculative
one), then `warmup` + `iters` runs of each kind over the same blobs, each between two events on the stream; nothing
synchronises the host inside the timed region -- the events are read after the last run.  The C ABI is called directly
with outputs allocated once, so a timed region holds the entry points' launches and the ctypes calls, no allocation.
  contribution  zero fill of the frame rows + k_contribution_tile + k_contribution_finish (all four outputs);
  walk          gsr_contribution alone (zero fill + k_contribution_tile);
  backward      gsr_backward with dL_dpix = 1 on channel 0 and dL_dacc = 0 (tile order, blend backward, gather,
                per-Gaussian backward): dL_dcolors[:, 0] is the weight sum; it gives neither the count nor the maximum;
  blend_fwd     the forward's own blend kernel(s), from the library's event profiler over `iters` further forwards
                (per frame, over up to ten frames: a near/far frame launches the kernel twice).
Prints one JSON line per shape: min / median / max in milliseconds and the ratios of the medians.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import gs_livm_amd as G  # noqa: E402
from gs_livm_amd import synthetic as S  # noqa: E402
from helpers import hip_forward  # noqa: E402

SHAPES = {"C3_2M_1920x1080": S.CONFIGS["C3"], "product_300k_640x512": (300_000, 640, 512, 5)}


def _timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}


def run(name, P, W, H, seed, iters, warmup, dev):
    sc = S.make_scene(P, W, H, seed)
    sc["colors_precomp"] = np.random.default_rng(seed).uniform(0, 1, (P, 3)).astype(np.float32)
    sc["shs"] = None
    for _ in range(2):  # synchronous, then the product's speculative forward
        t, fwd = hip_forward(sc, dev, debug=False, near_far=True)
    R, _, _, _, radii, geom, binning, img = fwd
    torch.cuda.synchronize()
    split, n_near, n_far = G.last_near_far()
    key = int(getattr(R, "key", R))
    dcol = torch.zeros((3, H, W), device=dev)
    dcol[0] = 1.0
    dacc = torch.zeros((1, H, W), device=dev)
    e = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    o = dict(m2=e(P, 3), conic=e(P, 4), op=e(P), col=e(P, 3), m3=e(P, 3), sc=e(P, 3), rot=e(P, 4))
    rows = torch.empty((P, 2), dtype=torch.int64, device=dev)
    n_touched = torch.empty(P, dtype=torch.int32, device=dev)
    wsum, wmax = e(P), e(P)
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def walk():
        rc = L.gsr_contribution(P, key, W, H, p(geom), p(binning), p(img), p(rows), stream)
        assert rc == 0, L.gsr_last_error()

    def contribution():
        walk()
        rc = L.gsr_contribution_finish(P, p(rows), 1, 0.0, p(n_touched), p(wsum), p(wmax), p(mask), None, stream)
        assert rc == 0, L.gsr_last_error()

    def backward():
        rc = L.gsr_backward(P, 0, 0, key, p(t["bg"]), W, H, p(t["means3D"]), None, p(t["colors_precomp"]), p(t["scales"]), 1.0,
                            p(t["rotations"]), None, p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]),
                            float(sc["tanfovx"]), float(sc["tanfovy"]), p(radii), p(geom), p(binning), p(img), p(dcol),
                            p(dacc), p(o["m2"]), p(o["conic"]), p(o["op"]), p(o["col"]), p(o["m3"]), None, None, p(o["sc"]),
                            p(o["rot"]), 0, stream)
        assert rc == 0, L.gsr_last_error()

    res = {"shape": name, "P": P, "W": W, "H": H, "iters": iters, "warmup": warmup, "instances": int(R),
           "near_far": bool(split)}
    res["contribution_ms"] = _timed(contribution, iters, warmup)
    res["walk_ms"] = _timed(walk, iters, warmup)
    res["backward_ms"] = _timed(backward, iters, warmup)
    res["contribution_again_ms"] = _timed(contribution, iters, warmup)  # how far the clock drifted meanwhile
    # the two routes agree (the backward's sum is float32 in another order)
    contribution()
    backward()
    torch.cuda.synchronize()
    d = (wsum.double() - o["col"][:, 0].double()).abs()
    res["worst_abs_diff_to_backward"] = float(d.max())
    res["rows_touched"] = int((n_touched > 0).sum())
    res["rows_radii_positive"] = int((radii > 0).sum())
    res["rows_weight_max_below_0.01"] = int(((n_touched > 0) & (wmax < 0.01)).sum())
    G.profile_enable(True, only=["k_blend_forward"])
    frames = min(iters, 10)  # (each of these forwards uploads the scene again)
    for _ in range(frames):
        hip_forward(sc, dev, debug=False, near_far=True)
    torch.cuda.synchronize()
    ms, launches = G.profile_read()["k_blend_forward"]
    G.profile_enable(False)
    res["blend_fwd_ms_per_frame"] = round(ms / frames, 4)
    res["blend_fwd_launches_per_frame"] = round(launches / frames, 2)
    both = 0.5 * (res["contribution_ms"]["median"] + res["contribution_again_ms"]["median"])
    res["contribution_over_backward"] = round(both / res["backward_ms"]["median"], 4)
    res["contribution_over_blend_fwd"] = round(both / max(res["blend_fwd_ms_per_frame"], 1e-9), 4)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, (P, W, H, seed) in SHAPES.items():
        line = json.dumps(run(name, P, W, H, seed, a.iters, a.warmup, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
