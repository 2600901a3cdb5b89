"""Times the weighted photometric loss (gsr_weighted_loss) beside the terms it extends, forward plus gradients.

    python tools/time_weighted_loss.py [--rounds 10] [--block 20] [--warmup 10] [--out FILE.jsonl]

Shapes: 3 x 1080 x 1920 and 3 x 512 x 640 (the product shape).  Variants, each one call between two device events:
  weighted_ones            weights = a tensor of ones, no gate, no exposure
  weighted_border          weights = a zero frame 12 pixels wide (an undistortion border)
  weighted_border_gate_exp the border, the gate acc >= 0.5 on a silhouette and an exposure
  weighted_absent_exp      no weights, no gate, an exposure: gsr_exposure_loss's work plus the two extra partials per
                           work unit, their re-sum in every workgroup of the backward and the finish's squared error
  exposure_loss            gsr_exposure_loss          photometric_loss   gsr_photometric_loss
  torch_route              m * img, m * gt, photometric_loss, times H W / S, autograd's backward to img (what a host
                           does without the fused term; allocations and Torch's launches included)
The fused variants call the C ABI directly with outputs and workspace allocated once: a timed region holds the entry
point's launches and the ctypes call.  Every variant is warmed up at the shape; then `rounds` rounds, each running a
block of `block` calls of every variant in turn, so that a drift of the clocks reaches all variants alike; nothing
synchronises the host inside a block.  Prints one JSON line per shape: min / median of each variant in milliseconds,
the medians over exposure_loss's, and microseconds per launch of three variants from the library's event profiler.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gs_livm_amd as G  # noqa: E402

SHAPES = {"3x1080x1920": (3, 1080, 1920), "3x512x640": (3, 512, 640)}


def variants(Cn, H, W, dev):
    g = torch.Generator().manual_seed(11)
    img = torch.rand((Cn, H, W), generator=g).to(dev)
    gt = (0.6 * torch.rand((Cn, H, W), generator=g).to(dev) + 0.4 * img.roll(1, 2)).clamp(0, 1)
    ones = torch.ones((H, W), device=dev)
    border = torch.zeros((H, W), device=dev)
    border[12:H - 12, 12:W - 12] = 1.0
    acc = torch.rand((H, W), generator=g).to(dev)
    e = torch.tensor([[0.8, -0.05], [1.0, 0.0], [1.25, 0.1]], device=dev)[:Cn].contiguous()
    win = G.reference_window_1d()
    taps = (C.c_float * 11)(*win.tolist())
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    nbytes = max(int(L.gsr_weighted_loss_workspace(Cn, H, W)), int(L.gsr_exposure_loss_workspace(Cn, H, W)),
                 int(L.gsr_photometric_loss_workspace(Cn, H, W)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out6, dimg, dexp = torch.empty(6, device=dev), torch.empty_like(img), torch.empty_like(e)

    def weighted(w, a, ex):
        def call():
            rc = L.gsr_weighted_loss(Cn, H, W, p(img), p(gt), p(w), p(a), 0.5, p(ex), taps, 0.2, p(out6), p(dimg),
                                     p(dexp) if ex is not None else None, p(ws), nbytes, stream)
            assert rc == 0, L.gsr_last_error()
        return call

    def exposure_loss():
        rc = L.gsr_exposure_loss(Cn, H, W, p(img), p(gt), p(e), taps, 0.2, p(out6), p(dimg), p(dexp), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    def photometric_loss():
        rc = L.gsr_photometric_loss(Cn, H, W, p(img), p(gt), taps, 0.2, p(out6), p(dimg), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    leaf = img.clone().requires_grad_(True)
    scale = float(H * W) / float(border.sum())

    def torch_route():
        leaf.grad = None
        (G.photometric_loss(border * leaf, border * gt, 0.2, win) * scale).backward()

    return dict(weighted_ones=weighted(ones, None, None), weighted_border=weighted(border, None, None),
                weighted_border_gate_exp=weighted(border, acc, e), weighted_absent_exp=weighted(None, None, e),
                exposure_loss=exposure_loss, photometric_loss=photometric_loss, torch_route=torch_route)


def run(name, shape, rounds, block, warmup, dev):
    v = variants(*shape, dev)
    for f in v.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in v}
    for _ in range(rounds):
        for k, f in v.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
            for a, b in ev:
                a.record()
                f()
                b.record()
            torch.cuda.synchronize()
            ms[k] += [a.elapsed_time(b) for a, b in ev]
    res = {"shape": name, "rounds": rounds, "block": block, "warmup": warmup}
    for k, t in ms.items():
        t.sort()
        res[k + "_ms"] = {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4)}
    # microseconds per launch from the library's event profiler, behind the timed blocks: the weighted kernels are
    # recorded under the exposure loss's ids, so each variant is profiled alone
    res["kernel_us"] = {}
    G.profile_read()
    for k in ("weighted_absent_exp", "weighted_border_gate_exp", "exposure_loss"):
        G.profile_enable(True)
        try:
            for _ in range(10):
                v[k]()
            torch.cuda.synchronize()
        finally:
            G.profile_enable(False)
        res["kernel_us"][k] = {n: round(1000.0 * t[0] / t[1], 2) for n, t in G.profile_read().items() if t[1]}
    base = res["exposure_loss_ms"]["median"]
    res["median_over_exposure_loss"] = {k: round(res[k + "_ms"]["median"] / base, 4) for k in ms}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, shape in SHAPES.items():
        line = json.dumps(run(name, shape, a.rounds, a.block, a.warmup, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
