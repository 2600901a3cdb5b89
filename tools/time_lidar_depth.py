"""Times the fused LiDAR depth supervision (gsr_lidar_depth_image once per keyframe; gsr_lidar_depth_loss with both
gradients per view per iteration) against the plain-Torch composition of the same term on the same device.

    python tools/time_lidar_depth.py [--iters 200] [--warmup 20] [--out FILE.jsonl]

Shape: 512 x 640 with a sweep of 100 000 points (tests/lidar_ref.py's recipe: 15 % of the points outside the image on
every side, one in sixteen behind the camera, the rpy pose).
  image        the C ABI called directly, the image and the counts allocated once: the ctypes call and its three launches
  loss         likewise: forward and both gradients, three launches, workspace allocated once
  torch_image  tests/lidar_ref.image_ops in float32 on the device: the projection in column arithmetic, the masks,
               scatter_reduce(amin) into an image of +inf and the conversion of the untouched pixels to 0; the points,
               R, t and K uploaded ONCE beforehand, no count is read back
  torch_loss   tests/lidar_ref.loss_forward_ops in float32 followed by torch.autograd.grad towards depth and acc, Torch's
               caching allocator warm
Each call lies between two device events; nothing synchronises the host inside a timed block -- the events are read
after the block's last call.  Blocks alternate fused, torch, fused again (the second fused block shows the drift
meanwhile).  Prints one JSON line: min / median / max in milliseconds per route and torch over fused (median over the
mean of the two fused medians).  The two routes' images and losses are compared before anything is timed.
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
import lidar_ref as R  # noqa: E402

H, W, N_POINTS = 512, 640, 100_000


def scene():
    """lidar_ref.inputs' recipe at the timed shape (its cases are fixed shapes)."""
    R.CASES = R.CASES + (("timed", H, W, N_POINTS, "rpy", 100),)
    return R.inputs("timed")


def run(iters, warmup, dev):
    x = scene()
    L = G.lib()
    mat = lambda a, n: (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:n]])  # noqa: E731
    tcw, k9 = mat(x["T_cw"], 12), mat(x["K"], 9)
    pts = torch.from_numpy(x["points"]).to(dev)
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("depth", "acc", "lidar")}
    image, counts = torch.empty(H, W, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = int(L.gsr_lidar_depth_loss_workspace(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out3, gd, ga = torch.empty(3, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused_image():
        rc = L.gsr_lidar_depth_image(N_POINTS, p(pts), tcw, k9, H, W, x["min_depth"], x["max_depth"], p(image),
                                     p(counts), stream)
        assert rc == 0, L.gsr_last_error()

    def fused_loss():
        rc = L.gsr_lidar_depth_loss(H, W, p(t["depth"]), p(t["acc"]), p(t["lidar"]), x["acc_min"], x["lam"], p(out3),
                                    p(gd), p(ga), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    Tt, Kt = torch.from_numpy(x["T_cw"]).to(dev), torch.from_numpy(x["K"]).to(dev)
    d = t["depth"].clone().requires_grad_(True)
    a = t["acc"].clone().requires_grad_(True)
    keep = {}

    def torch_image():
        keep["image"] = R.image_ops(pts, Tt, Kt, H, W, x["min_depth"], x["max_depth"], dtype=torch.float32, device=dev,
                                    counts=False)

    def torch_loss():
        loss = R.loss_forward_ops(d, a, t["lidar"], x["acc_min"], x["lam"])[0]
        keep["g"] = torch.autograd.grad(loss, [d, a])
        keep["loss"] = loss

    fused_image(), fused_loss(), torch_image(), torch_loss()
    torch.cuda.synchronize()
    lf, lt = float(out3[0]), float(keep["loss"].detach())
    assert abs(lf - lt) <= 1e-4 * abs(lt), (lf, lt)
    differ = int(((image - keep["image"]).abs() > 1e-4).sum())  # (beyond the rounding of z: another point won the pixel)
    assert differ <= 0.01 * H * W, differ                       # (points within a rounding of a pixel boundary)
    res = {"H": H, "W": W, "points": N_POINTS, "iters": iters, "warmup": warmup, "loss_fused": lf, "loss_torch": lt,
           "kept": int(counts[0]), "hit": int(counts[1]), "image_pixels_that_differ": differ,
           "device": torch.cuda.get_device_name(0)}
    for kind, fns in (("fused", (fused_image, fused_loss)), ("torch", (torch_image, torch_loss)),
                      ("fused_again", (fused_image, fused_loss))):
        for part, fn in zip(("image", "loss"), fns):
            for _ in range(warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            res["%s_%s_ms" % (kind, part)] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4),
                                              "max": round(ms[-1], 4)}
    for part in ("image", "loss"):
        both = 0.5 * (res["fused_%s_ms" % part]["median"] + res["fused_again_%s_ms" % part]["median"])
        res["torch_over_fused_%s_median" % part] = round(res["torch_%s_ms" % part]["median"] / both, 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    line = json.dumps(run(a.iters, a.warmup, torch.device("cuda:0")))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
