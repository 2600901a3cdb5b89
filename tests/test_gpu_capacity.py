"""Binning capacities at exact run ends (run with -m gpu on an MI355X).

A speculative forward sizes its binning blob before the instance count is known; when the count exceeds the capacity
the emitters stop at the capacity and the host redoes the frame.  Where they stop is read from the chunk tables
(BinningState::chunk_first / chunk_firstB): the last chunk's upper entry belongs to the run in which the capacity falls.
Whether the capacity cuts a run, ends one exactly or lies beyond the count are different code paths, so capacities here
are placed on run ends derived from the frame itself, not guessed.

Every binning blob of this module comes from the allocator filled with 0xFF bytes: a table entry the frame did not write
is then an out-of-range index, which the emitters' guard refuses and counts (gsr_emit_guard_trips) -- instead of
reading whatever the caching allocator's previous frame left there.
"""
import os
import re

import numpy as np
import pytest
import torch

import gs_livm_amd as G
from gs_livm_amd import synthetic as S
from helpers import check_near_far_against_one_chain, hip_backward, hip_forward

pytestmark = pytest.mark.gpu

EMIT_CHUNK = 2048   # slots per emitter workgroup (gsr_internal.hpp)
FAR_MIN_CAP = 4096  # a forced far capacity below this is raised to it (api.hip)


@pytest.fixture(autouse=True)
def poisoned_blobs(monkeypatch):
    """Every blob allocated while a test runs is filled with 0xFF on the current stream (the forward's) before the
    library gets its pointer."""
    alloc = G._capi._Blob._alloc

    def poisoned(self, ctx, nbytes):
        ptr = alloc(self, ctx, nbytes)
        if ptr:
            try:
                self.tensor.fill_(0xFF)
            except Exception:  # pragma: no cover - surfaces as GSR_ERR_ALLOC
                return None
        return ptr

    monkeypatch.setattr(G._capi._Blob, "_alloc", poisoned)
    yield


def _depth_position(v, P):
    order = v["depth_order"].long().cpu().numpy()
    pos = np.empty(P, np.int64)
    pos[order] = np.arange(P)
    return order, pos


def far_runs(v, P):
    """(Gaussian ids, run lengths) of a split frame's far chain in slot order: the Gaussians in the far segments of the
    tile lists, in depth order, each with its whole tile rectangle."""
    assert v["near_far"]
    r = v["ranges"].long().cpu().numpy()
    rn = v["ranges_near"].long().cpu().numpy()
    pl = v["point_list"].cpu().numpy()
    ln = rn[:, 1] - rn[:, 0]
    nfar = (r[:, 1] - r[:, 0]) - ln
    start = r[:, 0] + ln
    idx = np.repeat(start - (np.cumsum(nfar) - nfar), nfar) + np.arange(int(nfar.sum()))
    ids = np.unique(pl[idx])
    _, pos = _depth_position(v, P)
    ids = ids[np.argsort(pos[ids], kind="stable")]
    n = v["tiles_touched"].long().cpu().numpy()[ids]
    assert int(nfar.sum()) == int(n.sum()) == v["counters"][8], (int(nfar.sum()), int(n.sum()), v["counters"][8])
    assert len(ids) == v["counters"][10]
    return ids, n


def one_chain_runs(v, P, R):
    """(Gaussian ids, run lengths) of a one-chain frame: every Gaussian with instances, in depth order."""
    order, _ = _depth_position(v, P)
    n = v["tiles_touched"].long().cpu().numpy()[order]
    ids, n = order[n > 0], n[n > 0]
    assert int(n.sum()) == R
    return ids, n


def _end_between_long_runs(lengths, lo, hi, multiple=False):
    """A run end E with lo <= E < hi, E a multiple of EMIT_CHUNK or not; off the multiple, the runs on both sides of E
    are at least two slots long (E - 1 and E + 1 then lie strictly inside runs)."""
    ends = np.cumsum(lengths)
    for k in range(len(ends) - 1):
        E = int(ends[k])
        if not lo <= E < hi:
            continue
        if multiple:
            if E % EMIT_CHUNK == 0:
                return E
        elif E % EMIT_CHUNK != 0 and lengths[k] >= 2 and lengths[k + 1] >= 2:
            return E
    raise AssertionError("no run end in [%d, %d) of the wanted kind (multiple of %d: %s)" % (lo, hi, EMIT_CHUNK, multiple))


def _inside_long_run(lengths, lo, hi):
    """A slot strictly inside the longest run that lies in [lo, hi)."""
    ends = np.cumsum(lengths)
    starts = ends - lengths
    ok = (starts >= lo) & (ends < hi) & (lengths >= 3)
    assert ok.any(), "no run of >= 3 slots in [%d, %d)" % (lo, hi)
    k = int(np.argmax(np.where(ok, lengths, 0)))
    return int(starts[k] + lengths[k] // 2)


def _classify(c, lengths):
    ends = np.cumsum(lengths)
    if c > int(ends[-1]):
        return "beyond the count"
    return "run end" if c in set(ends.tolist()) else "inside a run"


def capacity_cases(lengths, lo):
    """(capacity, where it claims to sit) for a chain whose runs have these lengths: run ends at and off an EMIT_CHUNK
    multiple, their neighbours, a slot inside a long run, and the count itself with its neighbours."""
    R = int(np.sum(lengths))
    E = _end_between_long_runs(lengths, lo, R - 2)
    E2 = _end_between_long_runs(lengths, lo, R - 2, multiple=True)
    cases = [(E, "run end"), (E - 1, "inside a run"), (E + 1, "inside a run"),
             (_inside_long_run(lengths, lo, R), "inside a run"), (E2, "run end")]
    for c in (R - 1, R):
        cases.append((c, _classify(c, lengths)))
    cases.append((R + 1, "beyond the count"))
    for c, where in cases:
        assert c >= lo and _classify(c, lengths) == where, (c, where, _classify(c, lengths))
    assert cases[-2] == (R, "run end")
    return cases


def _far_scene():
    """A sparse scene (no tile ever saturates: the near chain leaves every tile live and the far chain does most of the
    work) whose farther half are tiny splats: one tile each, so the far chain has a run end at almost every slot there,
    and EMIT_CHUNK multiples among them; the nearer half has runs of many tiles."""
    sc = S.make_scene(40_000, 500, 300, 6, sh_degree=1)
    z = sc["means3D"][:, 2]
    sc["scales"][z > np.median(z)] = 0.0005
    return sc


FAR_NEAR_ENTRIES = 8


def _far_sweep(speculate_far):
    dev = torch.device("cuda:0")
    sc = _far_scene()
    P = sc["means3D"].shape[0]
    trips = G.emit_guard_trips()
    try:
        # the far runs of this near budget, from a frame that did not overflow
        G.set_binning_capacity_hint(0)
        hip_forward(sc, dev, debug=False)
        G.set_near_far_hints(FAR_NEAR_ENTRIES, None)
        _, fwd = hip_forward(sc, dev, debug=False, near_far=True)
        torch.cuda.synchronize()
        v = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], sc["W"], sc["H"])
        _, lengths = far_runs(v, P)
        RB = int(lengths.sum())
        assert RB > 3 * FAR_MIN_CAP, RB
        cases = capacity_cases(lengths, FAR_MIN_CAP)
        for c, where in cases:
            st = check_near_far_against_one_chain(sc, dev, FAR_NEAR_ENTRIES, far_capacity=c, expect_redo=c < RB,
                                                  speculate_far=speculate_far)
            if c >= RB:
                assert st["far"] == RB and st["live_tiles"] == st["tiles"], (c, where, st)
            torch.cuda.synchronize()
            assert G.emit_guard_trips() == trips, (c, where)
    finally:
        G.set_near_far_hints(None, None)
        G.set_far_speculation(None)
    return cases


@pytest.mark.parametrize("speculate_far", [True, False], ids=["speculated", "enqueued-outright"])
def test_far_capacity_at_run_ends(speculate_far, gpu_device):
    """Far capacities (gsr_set_near_far_hints) on a far run end off and on an EMIT_CHUNK multiple, one slot either side
    of it, inside a long run, and at the far count -1 / +0 / +1.  Each frame equals its one-chain frame bit for bit
    (images, n_contrib, final_T, every gradient), overflows -- and is redone -- exactly when the capacity is below the
    far count, and no emitter refuses its chunk table.  Far-chain speculation forced on (an asynchronous frame where
    the device has stream-side waits: the near chain leaves tiles live, so its far chain runs) and off."""
    cases = _far_sweep(speculate_far)
    assert len(cases) == 8


def test_far_capacity_at_run_ends_host_decided(gpu_device):
    """The same sweep through the host-decided far chain (GSR_ASYNC_FAR=0, read once per process: child process)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import pytest\n"
            "sys.exit(pytest.main(['-q', '-p', 'no:cacheprovider', '-m', 'gpu', %r, '-k', 'test_far_capacity_at_run_ends "
            "and speculated']))\n") % (os.path.dirname(here), here, os.path.join(here, "test_gpu_capacity.py"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSR_ASYNC_FAR="0"), capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and re.search(r"^1 passed", out.stdout, re.M), (out.stdout + out.stderr)[-3000:]


def test_one_chain_capacity_at_run_ends(gpu_device):
    """Binning capacities of a one-chain frame (gsr_set_binning_capacity_hint) on run ends off and on an EMIT_CHUNK
    multiple, around them, inside a long run and at R - 1 / R / R + 1: the frame and every gradient equal the
    synchronous frame's bit for bit, the overflow counter moves exactly below R, and no emitter refuses its chunk
    table."""
    dev = gpu_device
    P, W, H = 30_000, 400, 240
    sc = S.make_scene(P, W, H, 41, sh_degree=1)
    G.set_binning_capacity_hint(0)
    t, ref = hip_forward(sc, dev, debug=False)               # synchronous: key == count
    R = int(ref[0])
    assert ref[0].key == R
    v = G.state_views(ref[5], ref[6], ref[7], P, ref[0], W, H)
    _, lengths = one_chain_runs(v, P, R)
    cases = capacity_cases(lengths, 1)
    E2 = cases[4][0]
    cases += [(E2 - 1, _classify(E2 - 1, lengths)), (E2 + 1, _classify(E2 + 1, lengths))]
    dcol, dacc = S.make_upstream_grads(W, H, 41)
    gref = hip_backward(sc, t, ref, dcol, dacc, dev, debug=False)
    from test_gpu_parity import _same_frame
    trips = G.emit_guard_trips()
    for cap, where in cases:
        overflow = int(cap < R)
        before = G.speculation_stats()
        G.set_binning_capacity_hint(cap)
        t3, f3 = hip_forward(sc, dev, debug=False)
        st = G.speculation_stats()
        assert st["overflows"] - before["overflows"] == overflow, (cap, where)
        assert st["speculative_forwards"] == before["speculative_forwards"] + 1, (cap, where)
        assert f3[0].key == (R if overflow else cap) and int(f3[0]) == R, (cap, where)
        _same_frame(ref, f3, P, W, H, cap)
        g3 = hip_backward(sc, t3, f3, dcol, dacc, dev, debug=False)
        for k in gref:
            assert np.array_equal(gref[k], g3[k]), (cap, where, k)
        torch.cuda.synchronize()
        assert G.emit_guard_trips() == trips, (cap, where)


def test_several_threads_far_overflow_at_run_ends(gpu_device):
    """Three host threads (multiview.ViewThreads) render six views of the stack scene; after the warm-up iterations
    (speculative, split frames) one iteration forces each view's far capacity, on its worker thread, to an exact far
    run end of that view taken from a single-thread pass -- every frame of it overflows and is redone.  Images equal
    the single-thread run's bit for bit, gradients within the last bits, one overflow per view, no emitter refuses its
    chunk table."""
    from gs_livm_amd import multiview as MV
    from test_gpu_parity import _stack_scene
    dev = gpu_device
    W, H = 320, 208
    near_entries = 4
    g = _stack_scene(W=W, H=H)
    P = g["means3D"].shape[0]
    yaws = [-18.0, -12.0, -6.0, 6.0, 12.0, 18.0]
    bg = torch.ones(3, device=dev)
    caps, rasters = [], []
    try:
        for yaw in yaws:                                     # far run ends of each view, single thread
            sc = dict(g, **S.make_camera(W, H, yaw_deg=yaw), bg=np.ones(3, np.float32), scale_modifier=1.0,
                      colors_precomp=None, cov3D_precomp=None)
            G.set_binning_capacity_hint(0)
            hip_forward(sc, dev, debug=False)
            G.set_near_far_hints(near_entries, None)
            _, fwd = hip_forward(sc, dev, debug=False, near_far=True)
            torch.cuda.synchronize()
            v = G.state_views(fwd[5], fwd[6], fwd[7], P, fwd[0], W, H)
            _, lengths = far_runs(v, P)
            ends = np.cumsum(lengths)
            inner = ends[(ends >= FAR_MIN_CAP) & (ends < ends[-1])]
            assert len(inner), (yaw, int(ends[-1]))
            caps.append(int(inner[len(inner) // 2]))
    finally:
        G.set_near_far_hints(None, None)
    for yaw in yaws:
        cam = S.make_camera(W, H, yaw_deg=yaw)
        rasters.append(G.GaussianRasterizer(G.GaussianRasterizationSettings(
            H, W, cam["tanfovx"], cam["tanfovy"], bg, 1.0, torch.from_numpy(cam["viewmatrix"]).to(dev),
            torch.from_numpy(cam["projmatrix"]).to(dev), 0, torch.from_numpy(cam["campos"]).to(dev), False)))
    dcol, dacc = S.make_upstream_grads(W, H, 5)
    wc, wa = torch.from_numpy(dcol).to(dev), torch.from_numpy(dacc).to(dev)

    def call(r, m, leaves, cap):
        G.set_near_far_hints(near_entries, cap)              # (calling thread: the worker that renders this view)
        return r(leaves["means3D"], m, leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                 rotations=leaves["rotations"])

    def run(vt):
        leaves = {k: torch.from_numpy(g[k]).to(dev).requires_grad_(True)
                  for k in ("means3D", "scales", "rotations", "opacities", "shs")}
        for it in range(4):                                  # three iterations settle the histories, the fourth overflows
            forced = it == 3
            for v in leaves.values():
                v.grad = None
            sinks = [torch.zeros((P, 3), device=dev, requires_grad=True) for _ in rasters]
            calls = [lambda r=r, m=m, c=c: call(r, m, leaves, c if forced else None)
                     for r, m, c in zip(rasters, sinks, caps)]
            if forced:
                torch.cuda.synchronize()
                before = G.speculation_stats()
            outs = vt.render(calls) if vt is not None else [c() for c in calls]
            torch.autograd.backward([t for o in outs for t in (o[0], o[3])], [wc, wa] * len(outs))
            torch.cuda.synchronize()
            if forced:
                overflows = G.speculation_stats()["overflows"] - before["overflows"]
            images = [o[0].detach().clone() for o in outs]
        return images, {k: v.grad.clone() for k, v in leaves.items()}, overflows

    trips = G.emit_guard_trips()
    try:
        img1, g1, ov1 = run(None)
        vt = MV.ViewThreads(3, dev)
        try:
            img3, g3, ov3 = run(vt)
        finally:
            vt.close()
    finally:
        G.set_near_far_hints(None, None)                     # (the workers' settings ended with their threads)
    assert ov1 == ov3 == len(yaws), (ov1, ov3)
    for a, b in zip(img1, img3):
        assert torch.equal(a, b)
    for k in g1:
        scale = float(g1[k].abs().max())
        assert float((g1[k] - g3[k]).abs().max()) <= 2e-6 * scale + 1e-12, k
    assert G.emit_guard_trips() == trips
