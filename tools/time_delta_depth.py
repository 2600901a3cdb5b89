"""Times the fused delta-depth term (gsr_delta_depth_loss: forward and both depth gradients) against the float32
Torch-op restatement of the reference's ops on the same device.

    python tools/time_delta_depth.py [--iters 200] [--warmup 20] [--out FILE.jsonl]

Shapes: 640x512 (the product's frames) and 1920x1080.  Inputs: the synthetic pair of tests/delta_ref.py (smooth depth,
holes, masks, the 1.3 degree + 6 cm pose).
  fused   the C ABI called directly, outputs and workspace allocated once: a timed region holds the ctypes call and its
          four launches, no allocation.
  torch   tests/delta_ref.forward_ops in float32 on the device followed by torch.autograd.grad towards the two depth
          images: the reference's Torch ops one for one (src/gs/gaussian.cu:116-199, lioOptimization.cpp:1783-1799) and
          their autograd, with the three small matrices uploaded ONCE beforehand (the reference uploads them, and six
          more small tensors, on every iteration: the comparison favours the Torch route there) and Torch's caching
          allocator warm.
Each call lies between two events; nothing synchronises the host inside a timed block -- the events are read after the
block's last call.  Blocks alternate fused, torch, fused again (the second fused block shows the drift meanwhile).
Prints one JSON line per shape: min / median / max in milliseconds and torch over fused (median over the mean of the two
fused medians).  The two routes' losses are compared before anything is timed.
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
import delta_ref as D  # noqa: E402
import gs_livm_amd as G  # noqa: E402

SHAPES = {"640x512": (512, 640), "1920x1080": (1080, 1920)}


def pair(H, W):
    """delta_ref.inputs' recipe at any shape (its cases are fixed shapes)."""
    D.CASES = D.CASES + (("timed_%dx%d" % (H, W), H, W, "small", 100),)
    return D.inputs("timed_%dx%d" % (H, W))


def run(name, H, W, iters, warmup, dev):
    x = pair(H, W)
    L = G.lib()
    t = {k: torch.from_numpy(x[k]).to(dev) for k in ("depth_src", "acc_src", "depth_ref", "acc_ref")}
    mat = lambda a, n: (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float64).reshape(-1)[:n]])  # noqa: E731
    kin, kref, trel = mat(x["inv_K_src"], 9), mat(x["K_ref"], 9), mat(x["T_rel"], 12)
    nbytes = int(L.gsr_delta_depth_loss_workspace(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out3, gs, gr = torch.empty(3, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        rc = L.gsr_delta_depth_loss(H, W, p(t["depth_src"]), p(t["acc_src"]), p(t["depth_ref"]), p(t["acc_ref"]), kin,
                                    kref, trel, 0.2, p(out3), None, p(gs), p(gr), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    d_s = t["depth_src"][None].clone().requires_grad_(True)
    d_r = t["depth_ref"][None].clone().requires_grad_(True)
    a_s, a_r = t["acc_src"][None], t["acc_ref"][None]
    iK, Kr = (torch.from_numpy(np.asarray(x[k], np.float32)).to(dev) for k in ("inv_K_src", "K_ref"))
    T4 = torch.eye(4)
    T4[:3] = torch.from_numpy(np.asarray(x["T_rel"], np.float32))
    T4 = T4.to(dev)
    keep = {}

    def torch_route():
        loss = D.forward_ops(d_s, a_s, d_r, a_r, iK, Kr, T4, 0.2)[0]
        keep["g"] = torch.autograd.grad(loss, [d_s, d_r])
        keep["loss"] = loss

    fused()
    torch_route()
    torch.cuda.synchronize()
    lf, lt = float(out3[0]), float(keep["loss"].detach())
    assert abs(lf - lt) <= 1e-4 * abs(lt), (lf, lt)
    res = {"shape": name, "H": H, "W": W, "iters": iters, "warmup": warmup, "loss_fused": lf, "loss_torch": lt,
           "device": torch.cuda.get_device_name(0)}
    for kind, fn in (("fused", fused), ("torch", torch_route), ("fused_again", fused)):
        for _ in range(warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        res[kind + "_ms"] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}
    both = 0.5 * (res["fused_ms"]["median"] + res["fused_again_ms"]["median"])
    res["torch_over_fused_median"] = round(res["torch_ms"]["median"] / both, 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    for name, (H, W) in SHAPES.items():
        line = json.dumps(run(name, H, W, a.iters, a.warmup, dev))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
