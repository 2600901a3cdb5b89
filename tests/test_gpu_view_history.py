"""Rendered frames against the per-view history over keyframe sessions (run with -m gpu on an MI355X).

include/gsraster.h promises of everything a speculative forward predicts from -- the binning and far capacities, the
far-chain speculation's streak, the adaptive near budget, the pause of the split, the partial depth sort's flag --
that "a wrong guess costs a redo or a far chain, never a result".  The rest of the suite pins each decision by forcing
it through a hook on a view seen for the first time; here the history evolves on its own, as in production: cameras
keep their matrices, the model under them grows, is pruned and densified between frames, and no hook is called.  Every
frame of such a session is bit-identical to the same frame rendered synchronously in one chain (tests/view_history.py
has the sessions and the check; tests/test_view_history_cases.py holds their scenes to the oracle on the CPU).

Each session runs in a child process, once per variant of the knobs that are read once per process: a near budget of 24
entries per tile (every speculative frame of these sizes is split; asynchronous, host-decided and with the partial depth
sort) and the default environment (the same scripts through the one-chain capacity prediction).
"""
import os
import subprocess
import sys

import pytest

import view_history as V

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_child_died = []    # a child that faulted, aborted or hung: a finding to be read from the code, not run again


def _run_session(name, variant):
    if _child_died:
        pytest.fail("not started: an earlier session's child process died (%s)" % _child_died[0])
    code = ("import sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import view_history as V\nV.run_session(%r)\n") % (os.path.dirname(HERE), HERE, name)
    env = {k: v for k, v in os.environ.items() if k not in ("GSR_NEAR_ENTRIES", "GSR_ASYNC_FAR", "GSR_PRE_HIST_MIN_P")}
    env.update(V.ENV_VARIANTS[variant])
    try:
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired as e:
        _child_died.append("%s[%s]: no end after %d s" % (name, variant, e.timeout))
        tail = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
        pytest.fail("%s\n%s" % (_child_died[0], tail[-3000:]))
    text = out.stdout + out.stderr
    if out.returncode < 0 or out.returncode in (134, 139):
        _child_died.append("%s[%s]: exit status %d" % (name, variant, out.returncode))
        pytest.fail("%s\n%s" % (_child_died[0], text[-3000:]))
    for line in out.stdout.splitlines():
        if line.startswith("SESSION "):
            print(variant, line)
    assert out.returncode == 0 and "session ok" in out.stdout, text[-4000:]


@pytest.mark.parametrize("variant", list(V.ENV_VARIANTS))
def test_one_camera_changing_model(variant, gpu_device):
    """One camera in lock step over a model that loses its stack (a speculated miss, a raise of the budget on
    probation), grows until a capacity is outgrown (a redo), shrinks again for 70 frames (the 64-frame rules), is
    densified, and whose history is forgotten once mid-session."""
    _run_session("one_camera", variant)


@pytest.mark.parametrize("variant", list(V.ENV_VARIANTS))
def test_more_cameras_than_view_slots(variant, gpu_device):
    """Forty cameras, three rounds of all forwards then all backwards with nothing waiting in between: views are
    evicted and re-admitted while outcomes are pending, more than eight frames are in flight, and the model changes
    between the rounds."""
    _run_session("many_cameras", variant)


@pytest.mark.parametrize("variant", list(V.ENV_VARIANTS))
def test_same_matrices_other_frame(variant, gpu_device):
    """The same camera tensors at three image sizes, a camera that turns in place, and frames that alternate between
    the default stream and a side stream without a host wait."""
    _run_session("same_matrices", variant)
