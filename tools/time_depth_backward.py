"""Times the rasterizer's backward alone, without and with the depth gradient (gsr_backward / gsr_backward_depth).

    python tools/time_depth_backward.py [--iters 30] [--warmup 5] [--out FILE.jsonl]

Shapes: BASELINE C3 (2 M Gaussians, 1920x1080: the one-wave-per-tile blend kernel) and the product shape
(300 k Gaussians, 640x512: the wave-per-quad kernel).  One forward per shape, then `warmup` + `iters` backwards of
each kind over the same blobs (the backward leaves them clean), each between two events; nothing synchronises the host
inside the timed region -- the events are read after the last backward.  The C ABI is called directly with outputs
allocated once, so a timed region holds the entry point's launches (tile order where the forward left none, blend,
compaction, gather, per-Gaussian backward) and the ctypes call, no allocation and no fill.  Prints one JSON line per
shape: min / median / max of plain, depth and plain again in milliseconds, and depth over plain (median over the mean
of the two plain medians; min over the smaller plain min).
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


def run(name, P, W, H, seed, iters, warmup, dev):
    sc = S.make_scene(P, W, H, seed)
    for _ in range(2):  # synchronous, then the product's speculative forward
        t, fwd = hip_forward(sc, dev, debug=False, near_far=True)
    R, _, depth, _, radii, geom, binning, img = fwd
    dcol, dacc = (torch.from_numpy(a).to(dev) for a in S.make_upstream_grads(W, H, seed))
    gd = torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, (1, H, W)) / 40.0).astype(np.float32)).to(dev)
    M = int(t["shs"].shape[1])
    e = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    # outputs allocated once (the library overwrites every element); dL_dcov3D is not asked for, as in the autograd hosts
    o = dict(m2=e(P, 3), conic=e(P, 4), op=e(P), col=e(P, 3), m3=e(P, 3), sh=e(P, M, 3), sc=e(P, 3), rot=e(P, 4), dz=e(P))
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (P, int(sc["sh_degree"]), M, int(getattr(R, "key", R)), p(t["bg"]), W, H, p(t["means3D"]), p(t["shs"]), None,
            p(t["scales"]), 1.0, p(t["rotations"]), None, p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]),
            float(sc["tanfovx"]), float(sc["tanfovy"]), p(radii), p(geom), p(binning), p(img), p(dcol), p(dacc))
    outs = (p(o["m2"]), p(o["conic"]), p(o["op"]), p(o["col"]), p(o["m3"]), None, p(o["sh"]), p(o["sc"]), p(o["rot"]))

    def backward(with_depth):
        if with_depth:
            rc = L.gsr_backward_depth(*head, p(gd), *outs, p(o["dz"]), 0, stream)
        else:
            rc = L.gsr_backward(*head, *outs, 0, stream)
        assert rc == 0, L.gsr_last_error()

    res = {"shape": name, "P": P, "W": W, "H": H, "iters": iters, "warmup": warmup}
    # plain, depth, plain again: the second plain block shows how far the clock drifted meanwhile
    for kind, with_depth in (("plain", False), ("depth", True), ("plain_again", False)):
        for _ in range(warmup):
            backward(with_depth)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            backward(with_depth)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        res[kind + "_ms"] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}
    both = 0.5 * (res["plain_ms"]["median"] + res["plain_again_ms"]["median"])
    res["depth_over_plain_median"] = round(res["depth_ms"]["median"] / both, 4)
    res["depth_over_plain_min"] = round(res["depth_ms"]["min"] / min(res["plain_ms"]["min"], res["plain_again_ms"]["min"]), 4)
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
