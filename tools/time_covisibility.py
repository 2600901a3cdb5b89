"""Times keyframe covisibility on 2 M model rows (GPU): each fused call (csrc/covis.hip) against the same quantity in
Torch ops in the same process.  The Torch form keeps the visibility of K keyframes as a [K, P] bool tensor:
    pack          (radii > 0)                         one keyframe's row
    overlap 1:50  m[:1].float() @ m.float().T         with the counts m.sum(1)
    overlap 50:50 m.float() @ m.float().T             with the counts m.sum(1)
    count         m.sum(0)
    remap         m[:, keep]                          the columns a prune keeps
The bitsets hold the same information in P / 8 bytes per keyframe.
    python tools/time_covisibility.py [--rows 2000000] [--keyframes 50] [--iters 20] [--repeats 5] [--out profiles/covisibility_timing.json]
Device events around `iters` calls, the routes alternating within every repeat; medians and min..max of the repeats;
hip_device_us is the library's own event pair around the fused call's launches (k_visibility), from a run of its own.
Results of the two routes are compared once before anything is timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import gs_livm_amd as G
from gs_livm_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2_000_000)
ap.add_argument("--keyframes", type=int, default=50)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covisibility_timing.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
P, K = args.rows, args.keyframes
W = (P + 63) // 64


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


gen = torch.Generator().manual_seed(3)
# K keyframes that each see a share between 20 % and 60 % of the rows; the radii carry zeros and negative values
radii = torch.empty((K, P), dtype=torch.int32, device=dev)
for k in range(K):
    share = 0.2 + 0.4 * float(torch.rand((), generator=gen))
    seen = (torch.rand(P, generator=gen) < share).to(torch.int32)
    radii[k] = (torch.randint(1, 200, (P,), generator=gen, dtype=torch.int32) * seen).to(dev)
radii[:, ::97] *= -1
m = radii > 0                                           # the Torch form's state: [K, P] bool
slab = torch.empty((K, W), dtype=torch.int64, device=dev)
for k in range(K):
    G.visibility_pack(radii[k], out=slab[k])
dropped = (torch.rand(P, generator=gen) < 0.1).to(dev)  # a prune that drops a tenth of the rows
z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
rot = z(P, 4)
rot[:, 0] = 1.0
reasons, row_map, counts = _capi.prune_mark(z(P, 3), z(P, 3) - 3.0, rot, z(P, 1), drop=dropped)
P_new = int(counts[0])
keep = ~dropped
dst = torch.empty((K, W), dtype=torch.int64, device=dev)
row = torch.empty(W, dtype=torch.int64, device=dev)
tiles = lambda q: (q + 7) // 8  # noqa: E731

cases = {
    "pack": dict(hip=lambda: G.visibility_pack(radii[0], out=row), torch=lambda: radii[0] > 0,
                 hip_bytes=4 * P + 8 * W, torch_bytes=4 * P + P),
    "overlap_1_vs_%d" % K: dict(hip=lambda: G.covisibility(slab[0], slab),
                                torch=lambda: (m[:1].float() @ m.float().T, m[:1].sum(1), m.sum(1)),
                                hip_bytes=8 * W * (1 + tiles(1) * K), torch_bytes=(K + 1) * P * (1 + 4 + 4) + (K + 1) * P),
    "overlap_%d_vs_%d" % (K, K): dict(hip=lambda: G.covisibility(slab),
                                      torch=lambda: (m.float() @ m.float().T, m.sum(1)),
                                      hip_bytes=8 * W * (K + tiles(K) * K), torch_bytes=K * P * (1 + 4 + 4) + K * P),
    "count_%d" % K: dict(hip=lambda: G.observation_count(slab, P), torch=lambda: m.sum(0),
                         hip_bytes=8 * W * K + 4 * P, torch_bytes=K * P + 8 * P),
    "remap_%d" % K: dict(hip=lambda: G.visibility_remap(slab, reasons, row_map, dst=dst), torch=lambda: m[:, keep],
                         hip_bytes=8 * W * K * 2 + 4 * P + P, torch_bytes=K * P + K * P_new + P),
}

# the two routes compute the same quantity
inter, qc, kc = G.covisibility(slab)
mf = m.double()
same = dict(pack=torch.equal(G.visibility_pack(radii[0]), slab[0]),
            overlap=torch.equal(inter.double(), mf @ mf.T) and torch.equal(qc.long(), m.sum(1)) and torch.equal(qc, kc),
            count=torch.equal(G.observation_count(slab, P)[0].long(), m.sum(0)))
cut = m[:, keep]
G.visibility_remap(slab, reasons, row_map, dst=dst)
same["remap"] = all(torch.equal(G.visibility_pack(cut[k], words=W), dst[k]) for k in range(K))
del mf, cut
print(json.dumps(dict(P=P, K=K, P_new=P_new, same_as_torch=same)), flush=True)

rows = []
for name, c in cases.items():
    for _ in range(3):   # warm-up of both routes
        c["hip"]()
        c["torch"]()
    torch.cuda.synchronize()
    reps = [dict(hip_us=timed(c["hip"], args.iters), torch_us=timed(c["torch"], args.iters)) for _ in range(args.repeats)]
    # device time of the fused call alone (the library's event pair around its launches; a run of its own)
    G.profile_enable(True, only=["k_visibility"])
    for _ in range(args.iters):
        c["hip"]()
    ms, launches = G.profile_read()["k_visibility"]
    G.profile_enable(False)
    device_us = round(ms * 1e3 / max(launches, 1), 1)
    med = lambda k: round(statistics.median(x[k] for x in reps), 1)  # noqa: E731
    span = lambda k: [round(min(x[k] for x in reps), 1), round(max(x[k] for x in reps), 1)]  # noqa: E731
    r = dict(case=name, P=P, K=K, iters=args.iters, repeats=args.repeats, same_as_torch=same[name.split("_")[0]],
             hip_us=dict(median=med("hip_us"), span=span("hip_us")), hip_device_us=device_us,
             torch_us=dict(median=med("torch_us"), span=span("torch_us")),
             hip_bytes_moved=c["hip_bytes"], torch_bytes_moved=c["torch_bytes"],
             hip_GB_per_s=round(c["hip_bytes"] / (med("hip_us") * 1e-6) / 1e9, 1),
             torch_over_hip=round(med("torch_us") / med("hip_us"), 2))
    rows.append(r)
    print(json.dumps(r), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(rows, fh, indent=1)
    fh.write("\n")
