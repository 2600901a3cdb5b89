"""Times the robust LiDAR depth supervision: gsr_lidar_occlusion_filter (once per keyframe) against the Torch-op
composition of the same filter, and gsr_lidar_depth_loss_robust with both gradients (per view per iteration) against
gsr_lidar_depth_loss, on the same device in the same run.

    python tools/time_lidar_robust.py [--iters 300] [--warmup 30] [--repeats 5] [--out FILE.jsonl]

Shapes: 640 x 512 and 1920 x 1080.  Radius 2, tol 0.05 for the filter (tests/lidar_robust_ref.filter_image: a dense far
plane behind a sparse near surface); tests/lidar_robust_ref.PARAMS for the loss, on tests/lidar_ref.inputs' render recipe
over that image.
  filter        the C ABI called directly, output and counts allocated once: an 8-byte clear and one launch
  filter_no_counts  the same with a null counts2: the one launch alone
  torch_filter  tests/lidar_robust_ref.filter_ops in float32 on the device (where, max_pool2d, compare, where), Torch's
                caching allocator warm
  robust        forward and both gradients, three launches, workspace allocated once
  plain         gsr_lidar_depth_loss likewise: the same three images read, the same two written
Each call lies between two device events; nothing synchronises the host inside a timed block -- the events are read
after the block's last call.  A repeat times the four routes one after the other (robust and plain adjacent); the
repeats alternate them, and the spread of the repeats' medians is what a difference is held against.  Prints one JSON
line per shape: per route the median of every repeat, and the ratios of the medians of those.  The routes' results are
compared before anything is timed.
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
import lidar_robust_ref as R  # noqa: E402

SHAPES = ((512, 640), (1080, 1920))
RADIUS, TOL = 2, 0.05


def scene(H, W):
    """The structured LiDAR image and a render over it: A in [0.3, 1], D = A (z_L + an offset of up to +-0.4 m)."""
    rng = np.random.default_rng(H + W)
    zl = R.filter_image(H, W)
    with np.errstate(invalid="ignore"):
        zl = np.where((zl > 0) & np.isfinite(zl), zl, np.float32(0)).astype(np.float32)
    A = rng.uniform(0.3, 1.0, (H, W))
    off = rng.uniform(0.05, 0.4, (H, W)) * (rng.integers(0, 2, (H, W)) * 2 - 1)
    D = A * (np.where(zl > 0, zl, 5.0) + off)
    return zl, D.astype(np.float32), A.astype(np.float32)


def run(H, W, iters, warmup, repeats, dev):
    L = G.lib()
    raw = torch.from_numpy(R.filter_image(H, W)).to(dev)
    zl, D, A = (torch.from_numpy(a).to(dev) for a in scene(H, W))
    filtered, counts = torch.empty(H, W, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    nb_r, nb_p = int(L.gsr_lidar_depth_loss_robust_workspace(H, W)), int(L.gsr_lidar_depth_loss_workspace(H, W))
    ws_r, ws_p = torch.empty(nb_r, dtype=torch.uint8, device=dev), torch.empty(nb_p, dtype=torch.uint8, device=dev)
    out4, out3 = torch.empty(4, device=dev), torch.empty(3, device=dev)
    gd, ga = torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = R.PARAMS
    keep = {}

    def fused_filter():
        rc = L.gsr_lidar_occlusion_filter(H, W, p(raw), RADIUS, TOL, p(filtered), p(counts), stream)
        assert rc == 0, L.gsr_last_error()

    def fused_filter_no_counts():
        rc = L.gsr_lidar_occlusion_filter(H, W, p(raw), RADIUS, TOL, p(filtered), None, stream)
        assert rc == 0, L.gsr_last_error()

    def torch_filter():
        keep["filtered"] = R.filter_ops(raw, RADIUS, TOL)

    def robust():
        rc = L.gsr_lidar_depth_loss_robust(H, W, p(D), p(A), p(zl), 0.5, 0.7, q["huber_abs"], q["huber_rel"],
                                           q["clip_abs"], q["clip_rel"], p(out4), p(gd), p(ga), p(ws_r), nb_r, stream)
        assert rc == 0, L.gsr_last_error()

    def plain():
        rc = L.gsr_lidar_depth_loss(H, W, p(D), p(A), p(zl), 0.5, 0.7, p(out3), p(gd), p(ga), p(ws_p), nb_p, stream)
        assert rc == 0, L.gsr_last_error()

    routes = (("filter", fused_filter), ("filter_no_counts", fused_filter_no_counts), ("torch_filter", torch_filter),
              ("robust", robust), ("plain", plain))
    for _, fn in routes:
        fn()
    torch.cuda.synchronize()
    assert torch.equal(filtered.view(torch.int32), keep["filtered"].view(torch.int32))
    res = {"H": H, "W": W, "radius": RADIUS, "tol": TOL, "iters": iters, "warmup": warmup, "repeats": repeats,
           "kept": int(counts[0]), "removed": int(counts[1]), "supervised_share": round(float(out4[2]), 4),
           "clipped_share": round(float(out4[3]), 4), "device": torch.cuda.get_device_name(0)}
    med = {name: [] for name, _ in routes}
    for r in range(repeats):
        order = routes if r % 2 == 0 else routes[::-1]
        for name, fn in order:
            for _ in range(warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            med[name].append(round(ms[len(ms) // 2], 4))
    mid = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name in med:
        res[name + "_median_ms_per_repeat"] = med[name]
        res[name + "_ms"] = {"min": min(med[name]), "median": mid(med[name]), "max": max(med[name])}
    res["torch_over_fused_filter"] = round(mid(med["torch_filter"]) / mid(med["filter"]), 2)
    res["robust_over_plain"] = round(mid(med["robust"]) / mid(med["plain"]), 3)
    res["robust_over_plain_per_repeat"] = [round(a / b, 3) for a, b in zip(med["robust"], med["plain"])]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    for H, W in SHAPES:
        line = json.dumps(run(H, W, a.iters, a.warmup, a.repeats, torch.device("cuda:0")))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
