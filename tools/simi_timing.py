"""Times the fused LiDAR similarity loss against its Torch-op restatement on the GPU.

    python tools/simi_timing.py [--out profiles/simi_loss.jsonl]

m = 500 points against n = 8 000 and 32 000 selected Gaussians (scenes of tests/simi_ref.py), warm, 20 samples each,
torch.cuda.Event pairs around one call; the two sides alternate so that drift hits both.  Per size:
  fused        gsr_similarity_loss through the autograd node: forward + backward (loss, dL/dxyz, dL/dscaling)
  torch_f32    the restatement in float32 Torch ops, forward + backward: what the reference executes
  select_ref   the reference-style selection: per known key the rows appended to a host list and the points cat'ed,
               H2D, scatter_ into a mask, nonzero twice as calcSimiLoss does (each waits for the device), host clock
  select_index VoxelIndex.select (ranges on the host, two queued copies), host clock + one synchronise at the end
One process, no retry: a failure ends the script."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gs_livm_amd as G  # noqa: E402
import simi_ref as R  # noqa: E402

SAMPLES, WARM, LAM = 20, 5, 0.2


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=statistics.median(xs), min_ms=xs[0], max_ms=xs[-1],
                q1_ms=xs[len(xs) // 4], q3_ms=xs[(3 * len(xs)) // 4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simi_loss.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    lines = []
    for voxels in (500, 2000):
        sc = R.make_scene(voxels, 500, seed=77 + voxels)
        index = G.VoxelIndex(dev)
        index.add(sc["keys"], sc["counts"], 0)
        points, sel = index.select(sc["losses"], max_points=10 ** 9)
        xyz = torch.from_numpy(sc["xyz"]).to(dev).requires_grad_(True)
        scaling = torch.from_numpy(sc["scaling"]).to(dev).requires_grad_(True)

        def fused():
            loss = G.similarity_loss(points, sel, xyz, scaling, LAM)
            return torch.autograd.grad(loss, (xyz, scaling))

        def torch_f32():
            loss = R.similarity_loss_ref(points, sel, xyz, scaling, LAM)
            return torch.autograd.grad(loss, (xyz, scaling))

        def select_ref():
            rows, pts = [], torch.empty((0, 3))
            for k, p in sc["losses"].items():   # (the reference's loop: a row list and a growing cat per known key)
                if k in sc["index"]:
                    rows.extend(sc["index"][k])
                    pts = torch.cat([pts, p], 0)
            pts = pts.to(dev, non_blocking=True)
            t = torch.tensor(rows, dtype=torch.int32).long().to(dev, non_blocking=True)
            mask = torch.zeros(sc["P"], dtype=torch.long, device=dev)
            mask.scatter_(0, t, 1)
            return mask.nonzero().squeeze(1), mask.nonzero().squeeze(1)

        def select_index():
            return index.select(sc["losses"], max_points=10 ** 9)

        a, b = fused(), torch_f32()
        agree = float((a[0] - b[0]).abs().max())
        for _ in range(WARM):
            fused(); torch_f32(); select_ref(); select_index()
        t = {"fused": [], "torch_f32": [], "select_ref": [], "select_index": []}
        for _ in range(SAMPLES):
            t["fused"].append(event_ms(fused))
            t["torch_f32"].append(event_ms(torch_f32))
            t["select_ref"].append(host_ms(select_ref))
            t["select_index"].append(host_ms(select_index))
        rec = dict(m=int(points.shape[0]), n=int(sel.shape[0]), P=sc["P"], samples=SAMPLES, device=torch.cuda.get_device_name(0),
                   grad_xyz_max_abs_diff=agree, **{k: stats(v) for k, v in t.items()})
        rec["torch_over_fused"] = rec["torch_f32"]["median_ms"] / rec["fused"]["median_ms"]
        rec["select_ref_over_index"] = rec["select_ref"]["median_ms"] / rec["select_index"]["median_ms"]
        # not slower than the Torch sequence beyond the spread of the samples
        rec["fused_not_slower"] = rec["fused"]["median_ms"] <= rec["torch_f32"]["median_ms"] + (
            rec["torch_f32"]["q3_ms"] - rec["torch_f32"]["q1_ms"]) + (rec["fused"]["q3_ms"] - rec["fused"]["q1_ms"])
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["fused_not_slower"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
