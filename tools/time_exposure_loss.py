"""Times the exposure-compensated photometric loss against what a user writes without it, and against the plain loss,
on the same device, forward plus gradients through the Python autograd surface (GPU):

    python tools/time_exposure_loss.py [--iters 100] [--warmup 10] [--out FILE.json]

Shapes: 3 x 512 x 640 and 3 x 1080 x 1920 (tools/time_loss.py's inputs).  Routes:
  fused   exposure_photometric_loss(img, gt, e) and autograd towards img and e: three launches
  torch   the route before the fused term: g * img + b in Torch ops (e[:, 0, None, None] * img + e[:, 1, None, None])
          into photometric_loss, autograd towards img and e -- the compensated image written and read, the two
          elementwise nodes' backward, the two full-frame reductions
  plain   photometric_loss(img, gt) and autograd towards img: what the compensation is added to
Each call lies between two device events; nothing synchronises the host inside a timed block -- the events are read
after the block's last call.  Blocks alternate fused, torch, plain, and all three again (the second round shows the
drift meanwhile); a route's figure is the median over both of its blocks.  The routes' losses and gradients are compared
before anything is timed.  Prints one JSON document: min / median / max in milliseconds per route and shape, fused over
plain and torch over fused, and the microseconds per launch of the fused and the plain route's kernels from the library's
event profiler, taken behind the timed blocks.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gs_livm_amd as G  # noqa: E402

SHAPES = ((512, 640), (1080, 1920))


def routes(H, W, dev):
    gen = torch.Generator().manual_seed(1)
    img = torch.rand((3, H, W), generator=gen).to(dev).requires_grad_(True)
    gt = (0.6 * torch.rand((3, H, W), generator=gen).to(dev) + 0.4 * img.detach().roll(1, 2)).clamp(0, 1)
    e = torch.tensor([[0.8, -0.05], [1.0, 0.0], [1.25, 0.1]], device=dev).requires_grad_(True)
    keep = {}

    def fused():
        loss = G.exposure_photometric_loss(img, gt, e, 0.2)
        keep["fused"] = (loss,) + torch.autograd.grad(loss, (img, e))

    def torch_route():
        loss = G.photometric_loss(e[:, 0, None, None] * img + e[:, 1, None, None], gt, 0.2)
        keep["torch"] = (loss,) + torch.autograd.grad(loss, (img, e))

    def plain():
        loss = G.photometric_loss(img, gt, 0.2)
        keep["plain"] = (loss,) + torch.autograd.grad(loss, (img,))

    return dict(fused=fused, torch=torch_route, plain=plain), keep


def block(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def run(iters, warmup, dev):
    res = {"iters": iters, "warmup": warmup, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for H, W in SHAPES:
        fns, keep = routes(H, W, dev)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        lf, lt = float(keep["fused"][0].detach()), float(keep["torch"][0].detach())
        assert abs(lf - lt) <= 1e-5 * abs(lt), (lf, lt)   # (Torch's g * img + b need not be one FMA)
        # a sanity check that the routes compute one thing, not a bar (tests/test_gpu_exposure.py holds those): Torch
        # adds the millions of mixed-sign terms of dL/dg and dL/db in float32, and its g * img + b is two roundings, so
        # at a pixel where x' is within a rounding of gt the L1 term's sign may differ (a few pixels in millions)
        (fi, fe), (ti, te) = keep["fused"][1:], keep["torch"][1:]
        off = int(((fi - ti).abs() > 1e-3 * float(ti.abs().max())).sum())
        rel = [off / fi.numel(), float((fe - te).abs().max()) / float(te.abs().max())]
        assert rel[0] <= 1e-4 and rel[1] <= 5e-2, rel
        ms = {k: [] for k in fns}
        per_block = {k: [] for k in fns}
        for _ in range(2):
            for k, fn in fns.items():
                t = sorted(block(fn, iters, warmup))
                ms[k] += t
                per_block[k].append(round(t[len(t) // 2], 4))
        row = {"loss_fused": lf, "loss_torch": lt, "loss_plain": float(keep["plain"][0].detach()),
               "share_of_img_gradient_pixels_that_differ": rel[0], "exposure_gradient_difference_over_max": rel[1]}
        for k, t in ms.items():
            t.sort()
            row["%s_ms" % k] = {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4),
                                "block_medians": per_block[k]}
        # behind the timed blocks: the library's event profiler around ten calls of the fused and of the plain route
        # (each recorded launch costs a few microseconds of idle device, so these are not part of the figures above)
        G.profile_enable(True)
        for _ in range(10):
            fns["fused"]()
            fns["plain"]()
        torch.cuda.synchronize()
        G.profile_enable(False)
        row["kernel_us_per_launch"] = {k: round(ms * 1e3 / c, 2) for k, (ms, c) in sorted(G.profile_read().items()) if c}
        row["fused_over_plain_median"] = round(row["fused_ms"]["median"] / row["plain_ms"]["median"], 3)
        row["torch_over_fused_median"] = round(row["torch_ms"]["median"] / row["fused_ms"]["median"], 3)
        res["shapes"]["%dx%d" % (W, H)] = row
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    doc = json.dumps(run(a.iters, a.warmup, torch.device("cuda:0")), indent=1)
    print(doc, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")
