"""Times the sweep voxel map (gsr_voxel_sweep: four launches, no host wait inside) against a Torch-ops composition of
the same result on the same device.

    python tools/time_voxel_sweep.py [--iters 100] [--warmup 10] [--points 100000] [--fused-only] [--out FILE.jsonl]

Scene: `points` LiDAR returns on the six faces of a 6 x 5 x 3 m room with 4 mm of range noise -- about the surface
density of a 100 000-point sweep -- voxelised at the reference's config/basic_common.yaml values, grid 0.2 and
min_points 10.  Every timed call starts from an EMPTY table (zeroed in front of the first event), so each one inserts
every key, accumulates every point and seeds every voxel that matures: the most a single sweep can cost.
  fused   the C ABI called directly; table (sized as SweepVoxelMap sizes it: live + n <= capacity / 2), outputs, counts
          and workspace allocated once.  No count is read back inside the timed block.
  torch   floor and key in float64, torch.unique(return_inverse, return_counts), index_add_ of the first and second
          moments and the colours in float64, scatter_reduce(amin) + argsort for the order of first appearance,
          torch.linalg.eigh of the matured covariances, the clamp and V diag(lam) V^T.  torch.unique and the boolean
          mask WAIT for the device: the waits are part of the composition and inside the block.  (The moments are
          float64 sums: not the integer sums' bits, and not the same bits from run to run.)
Each call lies between two device events, read after the block's last call.  Blocks alternate fused, torch, fused again.
Prints one JSON line: min / median / max in milliseconds per route, torch over fused (median over the mean of the two
fused medians), the counts, and the bytes the insert's atomics add (14 64-bit adds and one 32-bit maximum per
accumulated point).  The share of the fused time spent in k_voxel_insert comes from a kernel trace of a --fused-only
run (profiles/README.md)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gs_livm_amd as G  # noqa: E402

GRID, MIN_POINTS, MIN_SIGMA = 0.2, 10, 0.001
Q = 1 << 20
LAUNCHES = 4   # insert, flag, scan, emit (csrc/voxel.hip)


def room(n, seed=0):
    r = np.random.RandomState(seed)
    size = np.array([6.0, 5.0, 3.0])
    face = r.randint(0, 6, n)
    p = r.uniform(0.0, 1.0, (n, 3)) * size
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = side * size[axis] + r.normal(0.0, 0.004, n)
    p -= size / 2
    cols = np.clip(127.0 + 40.0 * p, 0.0, 255.0)
    return p.astype(np.float32), cols.astype(np.float32)


def torch_ops(pts, cols, keep):
    n = pts.size(0)
    g = float(np.float32(GRID))
    t = pts.double() / g
    c = torch.floor(t)
    ok = (torch.isfinite(t) & (c.abs() < Q)).all(1)
    t, c, col = t[ok], c[ok], cols[ok].double()
    ci = c.long() + Q
    key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    q = torch.clamp(torch.floor((t - c) * Q), max=Q - 1)
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    m = uniq.numel()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=pts.device)  # noqa: E731
    s1 = z(m, 3).index_add_(0, inv, q)
    s2 = z(m, 9).index_add_(0, inv, (q[:, :, None] * q[:, None, :]).reshape(-1, 9))
    sc = z(m, 3).index_add_(0, inv, torch.clamp(torch.round(col * 256.0), 0.0, 65535.0))
    first = torch.full((m,), n, dtype=torch.long, device=pts.device).scatter_reduce_(
        0, inv, torch.arange(key.numel(), device=pts.device), "amin")
    mature = cnt >= MIN_POINTS
    order = torch.argsort(first[mature])
    k = cnt[mature][order].double()[:, None]
    a = s1[mature][order] / k
    unit = g / Q
    cov = (s2[mature][order] / k - (a[:, :, None] * a[:, None, :]).reshape(-1, 9)).reshape(-1, 3, 3) * (unit * unit)
    lam, V = torch.linalg.eigh(cov)
    lam = torch.clamp(lam.flip(1), min=float(np.float32(MIN_SIGMA)) ** 2)
    V = V.flip(2)
    keep["y"] = dict(xyz=((uniq[mature][order][:, None] >> torch.tensor([42, 21, 0], device=pts.device) & 0x1FFFFF) - Q
                          + (a + 0.5) / Q).mul(g).float(),
                     covs=((V * lam[:, None, :]) @ V.transpose(1, 2)).float(), rgbs=(sc[mature][order] / (256.0 * k)).float(),
                     scaling_raw=torch.log(torch.sqrt(lam)).float(), axes=V.float(), keys=uniq[mature][order],
                     matured=int(order.numel()), live=m)


def run(n, iters, warmup, fused_only, dev):
    L = G.lib()
    pts, cols = (torch.from_numpy(a).to(dev) for a in room(n))
    capacity = 1
    while 2 * n > capacity:
        capacity *= 2
    table = G._capi.voxel_table(capacity, dev)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)  # noqa: E731
    status, pkeys, keys = torch.empty(n, dtype=torch.uint8, device=dev), i64(n), i64(n)
    xyz, covs, rgb, scaling, rotation, normal = f32(n, 3), f32(n, 9), f32(n, 3), f32(n, 3), f32(n, 4), f32(n, 3)
    npoints, counts = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(6, dtype=torch.int32, device=dev)
    nbytes = int(L.gsr_voxel_sweep_workspace(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        rc = L.gsr_voxel_sweep(n, p(pts), p(cols), GRID, MIN_POINTS, MIN_SIGMA, 1.0, p(table), capacity, 0, p(status),
                               p(pkeys), p(xyz), p(covs), p(rgb), p(keys), p(npoints), p(scaling), p(rotation), p(normal),
                               p(counts), p(ws), nbytes, stream)
        assert rc == 0, L.gsr_last_error()

    keep = {}
    fused()
    torch.cuda.synchronize()
    cf = counts.tolist()
    res = {"points": n, "grid": GRID, "min_points": MIN_POINTS, "capacity": capacity, "iters": iters, "warmup": warmup,
           "counts_fused": cf, "fused_launches": LAUNCHES, "workspace_bytes": nbytes,
           "atomic_bytes": cf[0] * (14 * 8 + 4), "device": torch.cuda.get_device_name(0)}
    routes = [("fused", fused)]
    if not fused_only:
        torch_ops(pts, cols, keep)
        y = keep["y"]
        assert (y["matured"], y["live"]) == (cf[4], cf[5]), (y["matured"], y["live"], cf)
        assert torch.equal(y["keys"], keys[:cf[4]])
        res["max_xyz_difference"] = float((y["xyz"] - xyz[:cf[4]]).abs().max())
        routes += [("torch", lambda: torch_ops(pts, cols, keep)), ("fused_again", fused)]
    for kind, fn in routes:
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in [(None, None)] * warmup + ev:
            table.zero_()                      # an empty table for every call, outside the timed span
            if e0 is not None:
                e0.record()
            fn()
            if e1 is not None:
                e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        res["%s_ms" % kind] = {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}
    if not fused_only:
        both = 0.5 * (res["fused_ms"]["median"] + res["fused_again_ms"]["median"])
        res["torch_over_fused_median"] = round(res["torch_ms"]["median"] / both, 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    line = json.dumps(run(a.points, a.iters, a.warmup, a.fused_only, torch.device("cuda:0")))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
