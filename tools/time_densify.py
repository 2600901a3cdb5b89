"""Times adaptive density control (csrc/densify.hip) against the same two steps written as upstream's Torch ops on the
same device.

    python tools/time_densify.py [--iters 20] [--warmup 3] [--P 2000000] [--M 4] [--out FILE.jsonl]

Shape: P = 2 000 000 rows, M SH coefficients per channel, 60 % of the rows visible in the accumulated view, about 5 % of
the rows candidates, half of them big.
  accumulate        gsr_density_accumulate, the C ABI called directly: one launch
  densify           one GrowableGaussians.densify's device work and its one host wait on buffers allocated once: mark
                    (three launches), the copy of the offsets and counts, apply (one launch)
  torch_accumulate  upstream's add_densification_stats: the norm of the visible rows' gradient, two index-adds, and the
                    maximum of the radii
  torch_densify     upstream's densify_and_clone and densify_and_split (N = 2): the masks, torch.normal, build_rotation,
                    bmm, the cat of six leaves and twelve moments twice and the removal of the split parents from all
                    eighteen tensors; Torch's caching allocator warm
Each call lies between two device events; the statistics the fused densify consumes are restored outside the timed
block.  Blocks alternate fused, torch, fused again.  Prints one JSON line: min / median / max in milliseconds per route,
torch over fused, and the accumulate kernel's rate over its algorithmic bytes (16 B read per row, and a 12 B
read-modify-write -- 24 B -- per visible row).
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gs_livm_amd as G  # noqa: E402
from gs_livm_amd import _capi  # noqa: E402

GRAD_THRESHOLD, SIZE_THRESHOLD = 0.0002, 0.01


def build_rotation(q):
    q = torch.nn.functional.normalize(q)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_densify(leaves, m, v, accum, denom):
    """-> the eighteen tensors after densify_and_clone + densify_and_split"""
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    cand = grads.squeeze(1) >= GRAD_THRESHOLD
    big = torch.exp(leaves[3]).max(1).values > SIZE_THRESHOLD
    clone = cand & ~big
    grow = lambda ts, new: [torch.cat([t, n], 0) for t, n in zip(ts, new)]  # noqa: E731
    leaves2 = grow(leaves, [t[clone] for t in leaves])
    m2, v2 = (grow(s, [torch.zeros_like(t[clone]) for t in leaves]) for s in (m, v))
    split = torch.cat([cand & big, torch.zeros(int(clone.sum()), dtype=torch.bool, device=cand.device)])
    stds = torch.exp(leaves2[3][split]).repeat(2, 1)
    samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
    R = build_rotation(leaves2[4][split]).repeat(2, 1, 1)
    rep = lambda t: t[split].repeat(2, *([1] * (t.dim() - 1)))  # noqa: E731
    new = [torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + rep(leaves2[0]), rep(leaves2[1]), rep(leaves2[2]),
           torch.log(stds / 1.6), rep(leaves2[4]), rep(leaves2[5])]
    keep = ~torch.cat([split, torch.zeros(new[0].size(0), dtype=torch.bool, device=cand.device)])
    out = grow(leaves2, new) + grow(m2, [torch.zeros_like(t) for t in new]) + grow(v2, [torch.zeros_like(t) for t in new])
    return [t[keep] for t in out]


def run(iters, warmup, P, M, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(s, generator=gen, device=dev)  # noqa: E731
    u = lambda *s: torch.rand(s, generator=gen, device=dev)  # noqa: E731
    radii = torch.where(u(P) < 0.6, (u(P) * 40 + 1).int(), torch.zeros(P, dtype=torch.int32, device=dev))
    grad = r(P, 3) * 1e-4
    cand = u(P) < 0.05
    stats0 = torch.zeros(P, 3, device=dev)
    stats0[:, 1] = (u(P) * 5).floor() + 1
    stats0[:, 0] = torch.where(cand, 2.0, 0.5) * GRAD_THRESHOLD * stats0[:, 1]
    scaling = torch.where((u(P) < 0.5)[:, None], r(P, 3) * 0.3 - 6.0, r(P, 3) * 0.3 - 3.0)   # e^-6 < 0.01 < e^-3
    shapes = [(3,), (1, 3), (M - 1, 3), (3,), (4,), (1,)]
    L = G.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    stats = stats0.clone()

    def accumulate():
        rc = L.gsr_density_accumulate(P, p(radii), p(grad), p(stats), stream)
        assert rc == 0, L.gsr_last_error()

    # one mark to size the capacity buffers
    kinds, offsets, counts = _capi.densify_mark(stats0, scaling, GRAD_THRESHOLD, SIZE_THRESHOLD)
    n_new, n_clone, n_split = counts.tolist()
    cap = P + n_new
    base = [r(P, *s) for s in shapes]
    base[3] = scaling
    bufs = [[torch.zeros((cap,) + s, device=dev) for s in shapes] for _ in range(3)]
    dstats = torch.zeros(cap, 3, device=dev)

    def restore():
        for b, t in zip(bufs[0], base):
            b[:P].copy_(t)
        dstats[:P].copy_(stats0)

    def densify():
        k, o, _, both = _capi.densify_mark(dstats[:P], bufs[0][3][:P], GRAD_THRESHOLD, SIZE_THRESHOLD, packed=True)
        n = int(both.cpu()[P + 1])        # the one host wait
        _capi.densify_apply(P, n, k, o, 1, bufs[0], bufs[1], bufs[2], dstats)

    accum, denom = stats0[:, :1].clone(), stats0[:, 1:2].clone()
    max_radii = torch.zeros(P, device=dev)
    vis = radii > 0

    def torch_accumulate():
        accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
        denom[vis] += 1
        max_radii[vis] = torch.max(max_radii[vis], radii[vis].float())

    tm, tv = [torch.zeros_like(t) for t in base], [torch.zeros_like(t) for t in base]
    a0, d0 = stats0[:, :1].clone(), stats0[:, 1:2].clone()
    keep = {}

    def torch_upstream():
        keep["out"] = torch_densify(base, tm, tv, a0, d0)

    restore(), densify(), torch_upstream(), accumulate(), torch_accumulate()
    torch.cuda.synchronize()
    assert keep["out"][0].size(0) == cap, (keep["out"][0].size(0), cap)     # both routes add the same rows
    n_vis = int(vis.sum())
    res = {"P": P, "M": M, "visible": n_vis, "n_new": n_new, "n_clone": n_clone, "n_split": n_split, "iters": iters,
           "warmup": warmup, "device": torch.cuda.get_device_name(0)}
    for kind, fns in (("fused", (accumulate, densify)), ("torch", (torch_accumulate, torch_upstream)),
                      ("fused_again", (accumulate, densify))):
        for part, fn in zip(("accumulate", "densify"), fns):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for i in range(warmup + iters):
                if fn is densify:
                    restore()
                if i >= warmup:
                    ev[i - warmup][0].record()
                fn()
                if i >= warmup:
                    ev[i - warmup][1].record()
            torch.cuda.synchronize()
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            res["%s_%s_ms" % (kind, part)] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4),
                                              "max": round(ms[-1], 4)}
    for part in ("accumulate", "densify"):
        both = 0.5 * (res["fused_%s_ms" % part]["median"] + res["fused_again_%s_ms" % part]["median"])
        res["torch_over_fused_%s_median" % part] = round(res["torch_%s_ms" % part]["median"] / both, 2)
    nbytes = 16 * P + 24 * n_vis
    res["accumulate_algorithmic_bytes"] = nbytes
    res["accumulate_TBps_at_min"] = round(nbytes / (res["fused_accumulate_ms"]["min"] * 1e-3) / 1e12, 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=int, default=2_000_000)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    line = json.dumps(run(a.iters, a.warmup, a.P, a.M, torch.device("cuda:0")))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
