"""Times the fused point-to-plane loss (gsr_surfel_plane_loss: forward plus all three gradients) against the float32
Torch-ops restatement with autograd (tests/plane_ref.py) and against gsr_similarity_loss (forward plus both gradients)
on the same inputs.

    python tools/time_plane_loss.py [--iters 200] [--torch-iters 10] [--warmup 10] [--out FILE.jsonl]

Sizes (m points, n selected Gaussians): (500, 8000), the loop's cap on points and a typical selection, and
(3000, 50000).  Scenes: plane_ref.make_scene, the scenes of the tests; parameters lambda 0.2, huber 0.02, max_dist 0.05,
lambda_flat 0.3.  The C ABI is called directly with workspace and outputs allocated once, so a timed region holds the
three launches and the ctypes call, no allocation and no fill (the restatement allocates as Torch does: that is part of
what it costs).  Blocks run in the order fused, similarity, torch, fused again -- the second fused block shows how far
the clock drifted meanwhile.  Every call sits between two events, and one more pair spans the whole block; nothing
synchronises the host inside a block.  Prints one JSON line per size: min / median / max per call and the block's mean
in milliseconds, fused over similarity and torch over fused (medians; the fused median is the mean of its two blocks').
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
import plane_ref as PR  # noqa: E402

SIZES = {(500, 8000): (500, 16), (3000, 50000): (3125, 16)}
LAM, HUBER, MAX_DIST, LAMBDA_FLAT = 0.2, 0.02, 0.05, 0.3


def inputs(m, n, dev):
    voxels, per = SIZES[(m, n)]
    sc = PR.make_scene(voxels, m, seed=1000 + n + m, per_voxel=per)
    vi = G.VoxelIndex(dev)
    vi.add(sc["keys"], sc["counts"], 0)
    points, sel = vi.select(sc["losses"], max_points=10 ** 9)
    assert points.shape == (m, 3) and sel.shape == (n,)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return sc["P"], points, sel, t(sc["xyz"]), t(sc["scaling"]), t(sc["rotation"])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    whole[0].record()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    whole[1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4),
            "block_mean": round(whole[0].elapsed_time(whole[1]) / iters, 4), "iters": iters}


def run(m, n, iters, torch_iters, warmup, dev):
    P, points, sel, xyz, scaling, rotation = inputs(m, n, dev)
    L = G.lib()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    gx, gs, gr, out4, out3 = e(P, 3), e(P, 3), e(P, 4), e(4), e(3)
    nb_plane, nb_simi = int(L.gsr_surfel_plane_loss_workspace(m, n)), int(L.gsr_similarity_loss_workspace(m, n))
    ws = torch.empty(max(nb_plane, nb_simi), dtype=torch.uint8, device=dev)

    def fused():
        rc = L.gsr_surfel_plane_loss(P, m, n, p(points), p(sel), p(xyz), p(scaling), p(rotation), LAM, HUBER, MAX_DIST,
                                     LAMBDA_FLAT, p(out4), p(gx), p(gs), p(gr), 0, p(ws), nb_plane, stream)
        assert rc == 0, L.gsr_last_error()

    def simi():
        rc = L.gsr_similarity_loss(P, m, n, p(points), p(sel), p(xyz), p(scaling), LAM, p(out3), p(gx), p(gs), 0, p(ws),
                                   nb_simi, stream)
        assert rc == 0, L.gsr_last_error()

    leaves = [t.clone().requires_grad_(True) for t in (xyz, scaling, rotation)]

    def restated():
        loss = PR.plane_loss_ref(points, sel, *leaves, LAM, HUBER, MAX_DIST, LAMBDA_FLAT)
        return torch.autograd.grad(loss, leaves)

    res = {"m": m, "n": n, "P": P, "warmup": warmup, "workspace_bytes": nb_plane}
    res["fused_ms"] = timed(fused, iters, warmup)
    res["similarity_ms"] = timed(simi, iters, warmup)
    res["torch_ms"] = timed(restated, torch_iters, min(warmup, 3))
    res["fused_again_ms"] = timed(fused, iters, warmup)
    # the two agree on what they computed (the tests hold both to float64; this guards the timing's inputs)
    fused()
    want = restated()
    res["max_abs_diff_grad_rotation"] = float((gr - want[2]).abs().max())
    both = 0.5 * (res["fused_ms"]["median"] + res["fused_again_ms"]["median"])
    res["fused_over_similarity_median"] = round(both / res["similarity_ms"]["median"], 4)
    res["torch_over_fused_median"] = round(res["torch_ms"]["median"] / both, 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for m, n in SIZES:
        line = json.dumps(run(m, n, a.iters, a.torch_iters, a.warmup, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
