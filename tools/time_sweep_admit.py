"""Times the fused sweep admission (gsr_sweep_admit: five launches, no host wait inside) against the Torch-ops
composition of the same selection (tests/seed_ref.admit_ops in float32) on the same device.

    python tools/time_sweep_admit.py [--iters 100] [--warmup 10] [--out FILE.jsonl]

Shapes: 100 000 points at 640 x 512 and 1 000 000 points at 1920 x 1080 (tests/seed_ref.py's recipe: 8 % of the points
outside the image on every side, one in sixteen behind the camera, the rpy pose, a near surface over the left 30 %, a
render with a hole over the lower 38 %), each "full" (depth, acc, image with exposure and lidar_depth given) and
"bare" (depth and acc only: no image, no lidar_depth).
  fused   the C ABI called directly; the outputs, the counts and the workspace allocated once.  No count is read back
          inside the timed block: the call itself never waits for the device.
  torch   seed_ref.admit_ops in float32 on the device, everything uploaded once, Torch's caching allocator warm.  Its
          compaction is a nonzero, which WAITS for the device: the wait is part of the composition and inside the block.
Each call lies between two device events, read after the block's last call.  Blocks alternate fused, torch, fused again
(the second fused block shows the drift meanwhile).  Prints one JSON line per shape and variant: min / median / max in
milliseconds per route, torch over fused (median over the mean of the two fused medians) and the launches of the fused
call.  The two routes' counts are compared before anything is timed (they may differ by the few points within a
rounding of a threshold).
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
import seed_ref as R  # noqa: E402

SHAPES = ((512, 640, 100_000), (1080, 1920, 1_000_000))
LAUNCHES = 5   # clear, classify, resolve, scan, emit (csrc/seed.hip)


def scene(H, W, n, full):
    """seed_ref.inputs' recipe at a timed shape (its cases are fixed shapes)."""
    name = "timed_%dx%d_%s" % (W, H, "full" if full else "bare")
    R.CASES[name] = (H, W, n, "rpy", "lidar", 100, () if full else ("lidar", "image", "exposure"), {})
    return R.inputs(name)


def run(H, W, n, full, iters, warmup, dev):
    x = scene(H, W, n, full)
    L = G.lib()
    mat = lambda a, k: (C.c_float * k)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:k]])  # noqa: E731
    tcw, k9 = mat(x["T_cw"], 12), mat(x["K"], 9)
    t = {k: (None if x[k] is None else torch.from_numpy(x[k]).to(dev)) for k in ("points",) + R.OPTIONAL}
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)  # noqa: E731
    xyz, covs, rgb, index, pixel, z, counts = f32(n, 3), f32(n, 9), f32(n, 3), i32(n), i32(n), f32(n), i32(6)
    nbytes = int(L.gsr_sweep_admit_workspace(n, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        rc = L.gsr_sweep_admit(n, p(t["points"]), None, tcw, k9, H, W, x["min_depth"], x["max_depth"], p(t["depth"]),
                               p(t["acc"]), x["acc_min"], x["depth_tol"], p(t["lidar"]), x["radius"], x["occlusion_tol"],
                               p(t["image"]), p(t["exposure"]), x["footprint"], 1, p(xyz), p(covs), p(rgb), p(index),
                               p(pixel), p(z), None, p(counts), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    xd = dict(x, **{k: t[k] for k in t})
    xd["T_cw"], xd["K"] = torch.from_numpy(x["T_cw"]).to(dev), torch.from_numpy(x["K"]).to(dev)
    keep = {}

    def torch_ops():
        keep["y"] = R.admit_ops(xd, torch.float32, dev)

    fused(), torch_ops()
    torch.cuda.synchronize()
    cf, ct = counts.tolist(), keep["y"]["counts"].tolist()
    assert sum(cf) == n == sum(ct) and max(abs(a - b) for a, b in zip(cf, ct)) <= 1e-3 * n, (cf, ct)
    res = {"H": H, "W": W, "points": n, "variant": "full" if full else "bare", "iters": iters, "warmup": warmup,
           "counts_fused": cf, "counts_torch": ct, "fused_launches": LAUNCHES, "workspace_bytes": nbytes,
           "device": torch.cuda.get_device_name(0)}
    for kind, fn in (("fused", fused), ("torch", torch_ops), ("fused_again", fused)):
        for _ in range(warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        res["%s_ms" % kind] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}
    both = 0.5 * (res["fused_ms"]["median"] + res["fused_again_ms"]["median"])
    res["torch_over_fused_median"] = round(res["torch_ms"]["median"] / both, 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    for H, W, n in SHAPES:
        for full in (True, False):
            line = json.dumps(run(H, W, n, full, a.iters, a.warmup, torch.device("cuda:0")))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
