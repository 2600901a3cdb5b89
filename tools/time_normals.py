"""Times the normal-map kernels: the attribute walk beside the contribution walk it repeats, the surfel normals, and the
depth-normal consistency loss beside the float32 Torch-ops composition of the same formulas.

    python tools/time_normals.py [--iters 30] [--warmup 5] [--out FILE.jsonl]

Shapes: the product shape (300 k Gaussians, 640x512) and BASELINE C3 (2 M Gaussians, 1920x1080).  One forward per shape
(synchronous, then the product's speculative one), then `warmup` + `iters` runs of each kind over the same blobs, each
between two events on the stream; nothing synchronises the host inside the timed region -- the events are read after
the last run.  The C ABI is called directly with outputs allocated once, so a timed region holds the entry points'
launches and the ctypes calls, no allocation.
  contribution_walk  gsr_contribution (zero fill + k_contribution_tile): the yardstick -- the same visits, with integer
                     atomics per (tile, entry) in place of image stores;
  attr1 / attr3      gsr_blend_attributes with 1 and 3 channels (k_attribute_tile);
  normals            gsr_surfel_normals over all P rows;
  loss_fwd / loss    gsr_normal_consistency_loss without and with both gradients, on the forward's depth and acc and
                     the blended normal image;
  torch_fwd / torch  tests/normal_ref.loss on the same float32 device tensors (float32 sums), without and with
                     autograd's backward (the composition reads its supervised count on the host: one wait per call).
Prints one JSON line per shape: min / median / max in milliseconds and the ratios of the medians.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import gs_livm_amd as G  # noqa: E402
from gs_livm_amd import synthetic as S  # noqa: E402
from helpers import hip_forward  # noqa: E402
import normal_ref as NR  # noqa: E402

SHAPES = {"product_300k_640x512": (300_000, 640, 512, 5), "C3_2M_1920x1080": S.CONFIGS["C3"]}


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
    for _ in range(2):  # synchronous, then the product's speculative forward
        t, fwd = hip_forward(sc, dev, debug=False, near_far=True)
    R, _, depth, acc, radii, geom, binning, img = fwd
    torch.cuda.synchronize()
    key = int(getattr(R, "key", R))
    e = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
    rows = torch.empty((P, 2), dtype=torch.int64, device=dev)
    T = torch.as_tensor(sc["viewmatrix"]).t()[:3].contiguous().float()   # [R | t] of the transposed view matrix
    tcw = (C.c_float * 12)(*[float(v) for v in T.reshape(-1)])
    nrm, out1, out3c = e(P, 3), e(1, H, W), e(3, H, W)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc: rc == 0 or sys.exit(L.gsr_last_error().decode())  # noqa: E731

    def walk():
        ok(L.gsr_contribution(P, key, W, H, p(geom), p(binning), p(img), p(rows), stream))

    def normals():
        ok(L.gsr_surfel_normals(P, p(t["means3D"]), p(t["scales"]), p(t["rotations"]), tcw, p(nrm), stream))

    def attr1():
        ok(L.gsr_blend_attributes(P, key, W, H, 1, p(nrm), p(geom), p(binning), p(img), p(out1), stream))

    def attr3():
        ok(L.gsr_blend_attributes(P, key, W, H, 3, p(nrm), p(geom), p(binning), p(img), p(out3c), stream))

    fx, fy = W / (2.0 * sc["tanfovx"]), H / (2.0 * sc["tanfovy"])
    cam = (fx, fy, (W - 1) * 0.5, (H - 1) * 0.5)
    nbytes = int(L.gsr_normal_consistency_workspace(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    o3, gd, ga = e(3), e(H, W), e(H, W)
    kw = dict(acc_min=0.5, normal_min=0.1, jump_rel=0.05, lam=1.0)

    def loss(grads):
        ok(L.gsr_normal_consistency_loss(H, W, p(depth), p(acc), p(out3c), *cam, kw["acc_min"], kw["normal_min"],
                                         kw["jump_rel"], kw["lam"], p(o3), p(gd) if grads else None,
                                         p(ga) if grads else None, p(ws), nbytes, stream))

    d2, a2 = depth.view(H, W), acc.view(H, W)

    def torch_loss(grads):
        d = d2.detach().requires_grad_(grads)
        a = a2.detach().requires_grad_(grads)
        with torch.set_grad_enabled(grads), torch.device(dev):
            out = NR.loss(d, a, out3c, *cam, kw["acc_min"], kw["normal_min"], kw["jump_rel"], kw["lam"],
                          sum_dtype=torch.float32)[0]
            if grads:
                out[0].backward()

    normals()
    res = {"shape": name, "P": P, "W": W, "H": H, "iters": iters, "warmup": warmup, "instances": int(R),
           "near_far": bool(G.last_near_far()[0])}
    res["contribution_walk_ms"] = _timed(walk, iters, warmup)
    res["attr1_ms"] = _timed(attr1, iters, warmup)
    res["attr3_ms"] = _timed(attr3, iters, warmup)
    res["contribution_walk_again_ms"] = _timed(walk, iters, warmup)  # how far the clock drifted meanwhile
    res["normals_ms"] = _timed(normals, iters, warmup)
    res["loss_fwd_ms"] = _timed(lambda: loss(False), iters, warmup)
    res["loss_ms"] = _timed(lambda: loss(True), iters, warmup)
    res["torch_fwd_ms"] = _timed(lambda: torch_loss(False), iters, warmup)
    res["torch_ms"] = _timed(lambda: torch_loss(True), iters, warmup)
    loss(True)
    torch.cuda.synchronize()
    res["out3"] = [float(v) for v in o3.cpu()]
    both = 0.5 * (res["contribution_walk_ms"]["median"] + res["contribution_walk_again_ms"]["median"])
    res["attr1_over_contribution_walk"] = round(res["attr1_ms"]["median"] / both, 4)
    res["attr3_over_contribution_walk"] = round(res["attr3_ms"]["median"] / both, 4)
    res["torch_fwd_over_loss_fwd"] = round(res["torch_fwd_ms"]["median"] / res["loss_fwd_ms"]["median"], 2)
    res["torch_over_loss"] = round(res["torch_ms"]["median"] / res["loss_ms"]["median"], 2)
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
