"""Times the rasterizer's backward alone and followed by the camera pose gradient (gsr_backward, gsr_pose_gradient).

    python tools/time_pose_gradient.py [--iters 30] [--warmup 5] [--out FILE.jsonl] [--tree DIR] [--plain-only]

Shapes: BASELINE C3 (2 M Gaussians, 1920x1080) and the product shape (300 k Gaussians, 640x512), as
tools/time_depth_backward.py.  One forward per shape, then `warmup` + `iters` of each kind over the same blobs (the
backward leaves them clean), each between two events; nothing synchronises the host inside the timed region -- the
events are read after the last call.  The C ABI is called directly with outputs and the workspace allocated once.  Kinds:
plain (gsr_backward), pose (gsr_backward then gsr_pose_gradient), plain again (how far the clock drifted meanwhile), and
the pose gradient alone.  Prints one JSON line per shape: min / median / max in milliseconds, pose over plain (median
over the mean of the two plain medians; min over the smaller plain min) and the bytes the pose gradient reads per
visible Gaussian by its own count.

--tree DIR imports the package from another checkout (with --plain-only: one that has no pose gradient, the parent
commit), so that the unchanged default backward of two builds can be timed in alternating processes on one machine;
the spread between repeated runs of one build is the yardstick for a difference between two.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--label", default="")
ARGS = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])

sys.path.insert(0, os.path.abspath(ARGS.tree))
sys.path.insert(0, os.path.join(os.path.abspath(ARGS.tree), "tests"))
import gs_livm_amd as G  # noqa: E402
from gs_livm_amd import synthetic as S  # noqa: E402
from helpers import hip_forward  # noqa: E402

SHAPES = {"C3_2M_1920x1080": S.CONFIGS["C3"], "product_300k_640x512": (300_000, 640, 512, 5)}


def timed(fn, iters, warmup):
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


def run(name, P, W, H, seed, iters, warmup, dev, plain_only):
    sc = S.make_scene(P, W, H, seed)
    for _ in range(2):  # synchronous, then the product's speculative forward
        t, fwd = hip_forward(sc, dev, debug=False, near_far=True)
    R, _, _, _, radii, geom, binning, img = fwd
    dcol, dacc = (torch.from_numpy(a).to(dev) for a in S.make_upstream_grads(W, H, seed))
    M = int(t["shs"].shape[1])
    e = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    o = dict(m2=e(P, 3), conic=e(P, 4), op=e(P), col=e(P, 3), m3=e(P, 3), sh=e(P, M, 3), sc=e(P, 3), rot=e(P, 4))
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (P, int(sc["sh_degree"]), M, int(getattr(R, "key", R)), p(t["bg"]), W, H, p(t["means3D"]), p(t["shs"]), None,
            p(t["scales"]), 1.0, p(t["rotations"]), None, p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]),
            float(sc["tanfovx"]), float(sc["tanfovy"]), p(radii), p(geom), p(binning), p(img), p(dcol), p(dacc))
    outs = (p(o["m2"]), p(o["conic"]), p(o["op"]), p(o["col"]), p(o["m3"]), None, p(o["sh"]), p(o["sc"]), p(o["rot"]))

    def backward():
        rc = L.gsr_backward(*head, *outs, 0, stream)
        assert rc == 0, L.gsr_last_error()

    res = {"shape": name, "P": P, "W": W, "H": H, "iters": iters, "warmup": warmup, "label": ARGS.label,
           "visible": int((radii > 0).sum())}
    if plain_only:
        res["plain_ms"] = timed(backward, iters, warmup)
        res["plain_again_ms"] = timed(backward, iters, warmup)
        return res
    need = int(L.gsr_pose_gradient_workspace(P))
    ws, pose = torch.empty(need, dtype=torch.uint8, device=dev), e(6)

    def pose_gradient():
        rc = L.gsr_pose_gradient(P, W, H, p(t["means3D"]), p(t["scales"]), 1.0, p(t["rotations"]), None, p(t["viewmatrix"]),
                                 p(t["projmatrix"]), float(sc["tanfovx"]), float(sc["tanfovy"]), p(radii), p(o["m2"]),
                                 p(o["conic"]), None, p(o["m3"]), p(pose), p(ws), need, stream)
        assert rc == 0, L.gsr_last_error()

    def both():
        backward()
        pose_gradient()

    res["plain_ms"] = timed(backward, iters, warmup)
    res["pose_ms"] = timed(both, iters, warmup)
    res["plain_again_ms"] = timed(backward, iters, warmup)
    res["pose_alone_ms"] = timed(pose_gradient, iters, warmup)
    mean = 0.5 * (res["plain_ms"]["median"] + res["plain_again_ms"]["median"])
    res["pose_over_plain_median"] = round(res["pose_ms"]["median"] / mean, 4)
    res["pose_over_plain_min"] = round(res["pose_ms"]["min"] / min(res["plain_ms"]["min"], res["plain_again_ms"]["min"]), 4)
    # per row: the radius; per visible row: mean 12, scales 12, quaternion 16, dL_dmean2D.xy 8, dL_dconic.xyw 12, dL_dmean3D 12
    res["bytes_read"] = 4 * P + 72 * res["visible"]
    res["workspace_bytes"] = need
    res["dL_dpose"] = [float(x) for x in pose.cpu()]
    return res


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    for name, (P, W, H, seed) in SHAPES.items():
        line = json.dumps(run(name, P, W, H, seed, ARGS.iters, ARGS.warmup, dev, ARGS.plain_only))
        print(line, flush=True)
        if ARGS.out:
            with open(ARGS.out, "a") as f:
                f.write(line + "\n")
