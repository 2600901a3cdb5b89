"""The scenes and scripts of the keyframe sessions (tests/view_history.py, run by tests/test_gpu_view_history.py) have
the properties the sessions rely on -- with the CPU oracle alone."""
import numpy as np
import pytest

import view_history as V
from oracle import oracle as O


@pytest.fixture(scope="module")
def frames():
    """The oracle's frame (culled rectangles, as the product bins) of every scripted state and yaw the tests read."""
    O.set_threads(min(O.max_threads(), 8))
    out = {}
    for name, yaw in (("stack", 0.0), ("stack", 12.0), ("stack", 21.0), ("pruned", 0.0), ("grown", 0.0),
                      ("grown+stack", 0.0)):
        out[name, yaw] = O.forward(V.scene_of(V.state_gaussians(name), V.camera(yaw)), keep_handle=False, tight=True)
    for name in ("grown", "grown+stack"):           # the one-camera session's fainter large splats
        g = V.state_gaussians(name, n_grow=V.N_GROW_FAINT, opacity_scale=V.FAINT)
        out[name + ", faint", 0.0] = O.forward(V.scene_of(g, V.camera(0.0)), keep_handle=False, tight=True)
    return out


def _prediction(R):
    """the instance count a view predicts from a frame of R instances (include/gsraster.h; api.hip, plan_frame)"""
    return R * 5 // 4 + 65536


def test_instance_counts_keep_their_order(frames):
    R = {k: f.R for k, f in frames.items()}
    assert (R["stack", 0.0], R["stack", 12.0], R["stack", 21.0], R["pruned", 0.0]) == (26677, 24790, 23374, 10037)
    assert R["grown", 0.0] > R["stack", 0.0] > R["stack", 12.0] > R["stack", 21.0] > R["pruned", 0.0]
    assert R["grown+stack", 0.0] > R["grown", 0.0]
    # a capacity derived from the state before the growth as (R 5/4 + 65536) 5/4 cannot hold the grown frame, whatever
    # the rounding -- neither the pruned state's nor the stack's, which the view still remembers
    for grown in ("grown", "grown, faint"):
        for before in ("pruned", "stack"):
            assert R[grown, 0.0] > 1.5625 * R[before, 0.0] + 82_000
        # ... and the small states' prediction is below half of the grown one's (the high-water capacity is let go)
        for small in ("pruned", "stack"):
            assert 2 * _prediction(R[small, 0.0]) < _prediction(R[grown, 0.0])
    # at the budget of the variants every speculative frame is split (three budgets are below the prediction's floor),
    # at the default budget the grown frames are and the others are not
    tiles = (V.W // 16) * (V.H // 16)
    assert tiles == 260 and 3 * V.NEAR_ENTRIES * tiles < 65536
    for grown in ("grown", "grown, faint", "grown+stack", "grown+stack, faint"):
        assert _prediction(R[grown, 0.0]) >= 3 * 320 * tiles > _prediction(R["stack", 0.0])
    # ... the faint ones also after two raises of the budget by a quarter (the ratio is taken against the raised budget)
    for grown in ("grown, faint", "grown+stack, faint"):
        assert _prediction(R[grown, 0.0]) >= 3 * 480 * tiles
    # the far chain of the grown frame outgrows what a view derives from the far chains it has seen: half again as
    # much as the largest (at most every instance of the pruned frame) plus 131072
    for grown in ("grown", "grown, faint"):
        assert R[grown, 0.0] - (V.NEAR_ENTRIES + 1) * tiles > R["pruned", 0.0] * 3 // 2 + 131072


def test_the_stack_finishes_every_tile_at_yaw_0_only(frames):
    live0, n_near = V.live_tiles_after_near(frames["stack", 0.0], V.NEAR_ENTRIES)
    assert live0 == 0 and n_near == V.NEAR_ENTRIES          # 24 screen-filling splats are the whole near chain
    assert V.live_tiles_after_near(frames["stack", 21.0], V.NEAR_ENTRIES)[0] > 0
    assert V.live_tiles_after_near(frames["stack", 12.0], V.NEAR_ENTRIES)[0] > 0
    # put back behind the grown rows the stack still finishes everything; without it nothing finishes
    assert V.live_tiles_after_near(frames["grown+stack", 0.0], V.NEAR_ENTRIES)[0] == 0
    assert V.live_tiles_after_near(frames["pruned", 0.0], V.NEAR_ENTRIES)[0] == 260
    assert V.live_tiles_after_near(frames["grown", 0.0], V.NEAR_ENTRIES)[0] == 260
    # the faint large splats leave tiles live at the default budget too, and after the two raises (a quarter of the
    # budget each) under which their frames are still split; the stack in front of them finishes everything
    assert V.live_tiles_after_near(frames["grown, faint", 0.0], V.NEAR_ENTRIES)[0] == 260
    for entries in (320, 400, 480):
        assert V.live_tiles_after_near(frames["grown, faint", 0.0], entries)[0] >= 20, entries
        assert V.live_tiles_after_near(frames["grown+stack, faint", 0.0], entries)[0] == 0, entries
    assert V.live_tiles_after_near(frames["grown+stack, faint", 0.0], V.NEAR_ENTRIES)[0] == 0
    assert V.live_tiles_after_near(frames["grown", 0.0], 320)[0] == 0   # (as drawn they finish everything)


def test_turned_cameras_leave_what_the_sessions_expect():
    """The one-camera session's turn in place leaves a few tiles live at the budget and none at one and a half budgets
    (two raises of a quarter); the many-camera session's yaws up to 5 degrees leave none, its largest some."""
    g = V.state_gaussians("stack")
    fr = O.forward(V.scene_of(g, V.camera(V.TURN_DEG)), keep_handle=False, tight=True)
    assert 0 < V.live_tiles_after_near(fr, V.NEAR_ENTRIES)[0] < 26
    assert V.live_tiles_after_near(fr, V.NEAR_ENTRIES * 3 // 2)[0] == 0
    yaws = V.yaws_many()
    assert len(yaws) == 20 and min(yaws) == -21.0 and max(yaws) == 21.0 and sum(abs(y) <= 5.0 for y in yaws) >= 12
    for y in (5.0, -5.0, max(v for v in yaws if v <= 5.0)):
        fr = O.forward(V.scene_of(g, V.camera(y)), keep_handle=False, tight=True)
        assert V.live_tiles_after_near(fr, V.NEAR_ENTRIES)[0] == 0, y
    for y in (-21.0, 21.0, 15.0):
        fr = O.forward(V.scene_of(g, V.camera(y)), keep_handle=False, tight=True)
        assert V.live_tiles_after_near(fr, V.NEAR_ENTRIES)[0] > 0, y


@pytest.mark.parametrize("name", list(V.SESSIONS))
def test_scripts_are_deterministic_and_their_reference_pass_is_small(name):
    a, b = V.SESSIONS[name](7), V.SESSIONS[name](7)
    assert a == b and V.walk(a) == V.walk(b)
    assert V.SESSIONS[name](8) != a                         # (the seed reaches the growth, the densify and the rounds)
    frames, keys = V.walk(a)
    assert len(keys) <= 60, len(keys)                       # the reference pass renders each once
    assert len(frames) >= 40 and len({k[0] for k in keys}) >= 3   # at least three model states are shown
    assert sum(op[0] == "anchor" for op in a) >= 3
    if name == "many_cameras":
        cams = next(op[1] for op in a if op[0] == "cameras")
        assert len(cams) == 40 > 32 and all(-21.0 <= y <= 21.0 for y in cams)   # more views than slots
        assert all(len(op[1]) == 40 for op in a if op[0] == "round")


def test_the_large_splats_are_seeded():
    a, b = V.large_splats(50, 3), V.large_splats(50, 3)
    assert all(np.array_equal(a[k], b[k]) for k in V.KEYS)
    assert not np.array_equal(a["means3D"], V.large_splats(50, 4)["means3D"])
    assert (a["means3D"][:, 2] >= 1.0).all() and (a["means3D"][:, 2] <= 1.5).all() and (a["scales"] == 0.25).all()
