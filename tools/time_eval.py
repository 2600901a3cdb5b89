"""Times one frame's evaluation (GPU): image_metrics + one side-by-side pack + one depth pack, against the route the
library offered before csrc/metrics.hip -- photometric_loss(want_grad=False) for SSIM, the Torch ops of
gaussian_splatting::psnr and the Torch ops of the two 8-bit conversions, all on the device -- and k_metrics_forward
against k_loss_forward on the same image.
    python tools/time_eval.py [--iters 200] [--repeats 5] [--out profiles/eval_metrics_time.jsonl]
Device events around `iters` frames, the two routes alternating within every repeat; one JSON row per (shape, repeat)
and one summary row per shape (median and min..max of the repeats)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import gs_livm_amd as G

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_time.jsonl"))
args = ap.parse_args()
dev = torch.device("cuda:0")
WIN = G.reference_window_1d().tolist()


def fused(img, gt, depth):
    out4 = G._capi.image_metrics(img, gt, WIN)
    return out4, G.side_by_side(img, gt), G.depth_to_u8(depth, 50.0)


def torch_u8(t):   # tensor2CvMat3X's ops, on the device
    return t.permute(1, 2, 0).mul(255).clamp(0, 255).to(torch.uint8).flip(2)


def parent(img, gt, depth):
    out3, _ = G._capi.photometric_loss(img, gt, WIN, 0.2, want_grad=False)
    mse = (img - gt).pow(2).view(img.size(0), -1).mean(1, True)          # loss_utils.cuh:89-93
    psnr = (20.0 * torch.log10(1.0 / mse.sqrt())).mean()
    both = torch.cat([torch_u8(img), torch_u8(gt)], dim=1)
    d8 = (depth[0] * (255.0 / 50.0)).round().clamp(0, 255).to(torch.uint8)
    return (out3, psnr), both, d8


def timed(fn, a, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per frame


def kernels(a, only, n=20):
    G.profile_enable(True, only=only)
    for _ in range(n):
        fused(*a)
        parent(*a)
    torch.cuda.synchronize()
    G.profile_enable(False)
    return {k: ms * 1e3 / c for k, (ms, c) in G.profile_read().items() if c}


rows = []
for H, W in ((512, 640), (1080, 1920)):
    gen = torch.Generator().manual_seed(1)
    img = torch.rand((3, H, W), generator=gen).to(dev)
    gt = (0.6 * torch.rand((3, H, W), generator=gen).to(dev) + 0.4 * img.roll(1, 2)).clamp(0, 1)
    depth = (torch.rand((1, H, W), generator=gen) * 60.0).to(dev)
    a = (img, gt, depth)
    for _ in range(10):   # warm-up of every shape and route
        f, p = fused(*a), parent(*a)
    torch.cuda.synchronize()
    agree = dict(kind="agreement", H=H, W=W, psnr_fused=float(f[0][0]), psnr_torch=float(p[0][1]), ssim_fused=float(f[0][1]),
                 ssim_loss=float(p[0][0][2]), side_by_side_equal=bool(torch.equal(f[1], p[1])),
                 depth_bytes_differing=int((f[2] != p[2]).sum()))
    print(json.dumps(agree), flush=True)
    rows.append(agree)
    reps = []
    for r in range(args.repeats):
        t_new, t_old = timed(fused, a, args.iters), timed(parent, a, args.iters)
        k = kernels(a, ["k_metrics_forward", "k_loss_forward", "k_metrics_finalize", "k_pack_image_u8", "k_pack_depth_u8"])
        row = dict(kind="repeat", H=H, W=W, repeat=r, iters=args.iters, fused_us=round(t_new, 2), parent_route_us=round(t_old, 2),
                   kernel_us={n: round(v, 2) for n, v in sorted(k.items())})
        reps.append(row)
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = lambda f: round(statistics.median(f(x) for x in reps), 2)  # noqa: E731
    span = lambda f: [round(min(f(x) for x in reps), 2), round(max(f(x) for x in reps), 2)]  # noqa: E731
    summary = dict(kind="summary", H=H, W=W, repeats=args.repeats, iters=args.iters,
                   fused_us=dict(median=med(lambda x: x["fused_us"]), span=span(lambda x: x["fused_us"])),
                   parent_route_us=dict(median=med(lambda x: x["parent_route_us"]), span=span(lambda x: x["parent_route_us"])),
                   kernel_us={n: dict(median=med(lambda x, n=n: x["kernel_us"][n]), span=span(lambda x, n=n: x["kernel_us"][n]))
                              for n in reps[0]["kernel_us"]})
    rows.append(summary)
    print(json.dumps(summary), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    for row in rows:
        fh.write(json.dumps(row) + "\n")
