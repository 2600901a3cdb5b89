"""CPU tests of the host-side logic: operator-surface argument rules, synthetic scene / camera
conventions, view sharding and the two exchange steps over gloo with world_size 2."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gs_livm_amd as G
from gs_livm_amd import multiview as MV
from gs_livm_amd import synthetic as S


def _settings():
    cam = S.make_camera(64, 48)
    return G.GaussianRasterizationSettings(48, 64, cam["tanfovx"], cam["tanfovy"], torch.ones(3), 1.0,
                                           torch.from_numpy(cam["viewmatrix"]), torch.from_numpy(cam["projmatrix"]), 0,
                                           torch.from_numpy(cam["campos"]), False)


def test_rasterizer_argument_exclusivity():
    """src/gs/rasterizer.cu:161-169: exactly one of shs/colors and one of (scales,rotations)/cov3D."""
    r = G.GaussianRasterizer(_settings())
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        r(m, m, o, shs=None, colors_precomp=None, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        r(m, m, o, shs=torch.zeros(4, 1, 3), colors_precomp=m, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r(m, m, o, shs=torch.zeros(4, 1, 3))
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r(m, m, o, shs=torch.zeros(4, 1, 3), scales=m, rotations=torch.zeros(4, 4), cov3D_precomp=torch.zeros(4, 6))


def test_cpp_operator_surface_mirrors_the_reference():
    """csrc/torch_binding.cpp: same free functions / classes as src/gs/rasterize_points.cu + rasterizer.cu, and
    the same std::invalid_argument rules (rasterizer.cu:161-169), exercised through pybind11 (no GPU needed)."""
    T = G.torch_ops()
    for name in ("RasterizeGaussiansCUDA", "RasterizeGaussiansBackwardCUDA", "markVisible",
                 "GaussianRasterizationSettings", "GaussianRasterizer"):
        assert hasattr(T, name), name
    s = _settings()
    r = T.GaussianRasterizer(T.GaussianRasterizationSettings(48, 64, s.tanfovx, s.tanfovy, s.bg, 1.0, s.viewmatrix,
                                                            s.projmatrix, 0, s.camera_center, False))
    m, o = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        r.forward(m, m, o, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        r.forward(m, m, o, shs=torch.zeros(4, 1, 3), colors_precomp=m, scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r.forward(m, m, o, shs=torch.zeros(4, 1, 3))
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r.forward(m, m, o, shs=torch.zeros(4, 1, 3), scales=m, rotations=torch.zeros(4, 4),
                  cov3D_precomp=torch.zeros(4, 6))
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        T.RasterizeGaussiansCUDA(torch.ones(3), torch.zeros(4, 2), m, o, m, torch.zeros(4, 4), 1.0, torch.zeros(0),
                                 s.viewmatrix, s.projmatrix, 1.0, 1.0, 8, 8, torch.zeros(4, 1, 3), 0, s.camera_center,
                                 False, False)


def test_cpp_binding_exports_the_declared_members_as_strong_symbols():
    """The five members include/gs/gs/rasterizer.cuh:22-80 declares without bodies and the three functions of
    rasterize_points.cuh must be DEFINED (type T), not merely inlined: GS-LIVM's callers link against them."""
    import subprocess
    so = os.path.join(os.path.dirname(G.LIB_PATH), "_gsraster_torch.so")
    out = subprocess.check_output(["nm", "-DC", "--defined-only", so], text=True)
    strong = [ln.split(" ", 2)[2] for ln in out.splitlines() if len(ln.split(" ", 2)) == 3 and ln.split(" ", 2)[1] == "T"]
    for want in ("_RasterizeGaussians::forward(", "_RasterizeGaussians::backward(", "GaussianRasterizer::mark_visible(",
                 "GaussianRasterizer::rasterize_gaussians(", "GaussianRasterizer::forward(",
                 "RasterizeGaussiansCUDA(", "RasterizeGaussiansBackwardCUDA(", "markVisible("):
        assert any(s.startswith(want) for s in strong), want


@pytest.mark.skipif(not os.path.exists("/root/reference/include/gs/gs/rasterizer.cuh"),
                    reason="needs the reference tree (build container only)")
def test_cpp_binding_links_against_the_reference_headers():
    """INTEGRATION.md section 1, checked: torch_binding.cpp compiled against the reference's OWN rasterizer.cuh /
    rasterize_points.cuh (where they lie under /root/reference) links with a caller that sees only those headers, the
    program runs (host-side argument rules), and nm shows strong definitions for every declared member.
    Recipe: oracle/ref_link/ (outputs under oracle/_ref/, git-ignored; cached while the sources are unchanged)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", os.path.join(root, "oracle"), "ref_link"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "ref_link ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    txt = open(os.path.join(root, "oracle", "_ref", "link_check.txt")).read()
    assert txt.count("\n  T ") == 8 + 12 and "ref_link ok" in txt   # the rasterizer surface + gsr_torch_next.hpp


def test_forward_shape_error_like_reference():
    """src/gs/rasterize_points.cu:67-69"""
    with pytest.raises(ValueError, match=r"\(num_points, 3\)"):
        G.rasterize_forward(torch.ones(3), torch.zeros(4, 2), None, None, None, None, 1.0, None, None, None, 1, 1, 8,
                            8, None, 0, None)


def test_camera_conventions():
    cam = S.make_camera(1920, 1080, yaw_deg=15.0, position=(0.5, -0.2, 1.0))
    V, F = cam["viewmatrix"], cam["projmatrix"]
    assert np.allclose(V[:3, 3], 0) and V[3, 3] == 1  # transposed world->view: translation in the last ROW
    p = np.array([0.5, -0.2, 1.0, 1.0], np.float32)
    assert np.allclose(p @ V, [0, 0, 0, 1], atol=1e-6)  # camera centre maps to the view origin
    assert np.allclose(cam["campos"], [0.5, -0.2, 1.0], atol=1e-6)
    P = S.projection_matrix(S.ZNEAR, S.ZFAR, math.radians(60), math.radians(40))
    assert P[3, 2] == 1 and np.isclose(P[2, 2], 100 / 99.99) and np.isclose(P[2, 3], -1 / 99.99)  # camera.cu:66-76
    assert np.allclose(F, V @ S.projection_matrix(S.ZNEAR, S.ZFAR, math.radians(60), 2 * math.atan(
        math.tan(math.radians(30)) * 1080 / 1920)).T, atol=1e-6)
    assert np.isclose(cam["tanfovx"], math.tan(math.radians(30)))


def test_camera_mirror_has_the_reference_getters_and_matrices():
    """G.Camera = the rasterizer-facing part of the reference's Camera (src/gs/camera.cu:14-57): the tensors are the
    transposed matrices, full_proj = view @ projection, the centre is row 3 of the inverse view."""
    a = math.radians(-11.0)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32)
    fovx = math.radians(70.0)
    fovy = 2.0 * math.atan(math.tan(fovx / 2.0) * 480 / 640)
    cam = G.Camera(R, (0.3, -0.1, 0.7), fovx, fovy, 640, 480, device="cpu", uid=4, image_name="kf4")
    ref = S.make_camera(640, 480, fovx_deg=70.0, yaw_deg=-11.0, position=(0.3, -0.1, 0.7))
    # the rotation rows and every structural 0 / 1 are copies: bit-exact.  The translation row (-R^T T) and full_proj
    # are f32 dot products that torch and numpy round the way the host CPU's kernels sum them (FMA or not, in any
    # order): every such order lands within 1 ulp of the other
    V = cam.Get_world_view_transform().numpy()
    assert np.array_equal(V[:3], ref["viewmatrix"][:3]) and V[3, 3] == 1
    np.testing.assert_array_max_ulp(V, ref["viewmatrix"], maxulp=1)
    np.testing.assert_array_max_ulp(cam.Get_full_proj_transform().numpy(), ref["projmatrix"], maxulp=1)
    assert np.allclose(cam.Get_camera_center().numpy(), ref["campos"], atol=1e-6)
    assert (cam.Get_image_width(), cam.Get_image_height(), cam.Get_uid(), cam.Get_image_name()) == (640, 480, 4, "kf4")
    assert np.isclose(math.tan(cam.Get_FoVx() * 0.5), ref["tanfovx"]) and np.isclose(math.tan(cam.Get_FoVy() * 0.5),
                                                                                     ref["tanfovy"])
    P = G.get_projection_matrix(S.ZNEAR, S.ZFAR, fovx, fovy)  # the tensor = P transposed (Eigen memory, camera.cu:78-81)
    assert P[2, 3] == 1 and np.isclose(float(P[2, 2]), 100 / 99.99) and np.isclose(float(P[3, 2]), -1 / 99.99)
    assert np.array_equal(cam.Get_projection_matrix().numpy(), P.numpy())


def test_scene_generator_is_seeded_and_exercises_culls():
    a, b = S.make_scene(5000, 320, 240, 9, 1), S.make_scene(5000, 320, 240, 9, 1)
    assert all(np.array_equal(a[k], b[k]) for k in ("means3D", "scales", "rotations", "opacities", "shs"))
    assert np.allclose(np.linalg.norm(a["rotations"], axis=1), 1, atol=1e-6)
    assert 0.005 < (a["means3D"][:, 2] <= 0.2).mean() < 0.05 and 0.002 < (a["scales"] > 0.3).any(1).mean() < 0.03
    assert a["shs"].shape == (5000, 4, 3) and a["opacities"].min() >= 0.05


def test_shard_views_covers_every_view_once():
    for n in (0, 1, 3, 8, 11):
        for w in (1, 2, 4, 8):
            got = sorted(v for r in range(w) for v in MV.shard_views(n, r, w))
            assert got == list(range(n))


def test_gaussian_buffer_layout():
    g = S.make_gaussians(100, 3, sh_degree=1)
    buf = MV.GaussianBuffer(100, 4, "cpu").load(g)
    assert buf.flat.numel() == 100 * MV.floats_per_gaussian(4) and buf.nbytes() == 100 * 23 * 4
    assert MV.floats_per_gaussian(1) * 4 == 56 and MV.floats_per_gaussian(16) * 4 == 236
    want = dict(g, features_dc=g["shs"][:, :1], features_rest=g["shs"][:, 1:])
    for k, v in buf.views.items():
        assert v.data_ptr() >= buf.flat.data_ptr() and np.array_equal(v.numpy(), want[k])
    buf.views["opacities"].fill_(0.25)
    assert (buf.flat[100 * 22:100 * 23] == 0.25).all()


def test_reference_window_quirk():
    """loss_utils.cuh:24-31: floor((x - 11)/2) -> exponents 6,5,5,4,4,3,3,2,2,1,1: not symmetric."""
    w = G.reference_window_1d()
    k = np.array([6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1], np.float64)
    want = np.exp(-k * k / 4.5)
    want /= want.sum()
    assert np.allclose(w.numpy(), want, atol=1e-7) and abs(float(w.sum()) - 1) < 1e-6
    assert not np.allclose(w.numpy(), w.numpy()[::-1])



def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P, M = 500, 4
        buf = MV.GaussianBuffer(P, M, "cpu")
        if rank == 0:
            buf.load(S.make_gaussians(P, 17, sh_degree=1))
        MV.broadcast_gaussians(buf, src=0)
        want = S.make_gaussians(P, 17, sh_degree=1)
        want.update(features_dc=want["shs"][:, :1], features_rest=want["shs"][:, 1:])
        ok = all(np.array_equal(buf.views[k].numpy(), want[k]) for k in buf.views)
        # each rank "renders" its views: gradient = (view index + 1) everywhere; owner gets the sum
        mine = MV.shard_views(5, rank, world)
        grad = MV.GaussianBuffer(P, M, "cpu")
        for v in mine:
            grad.flat += float(v + 1)
        MV.reduce_gradients(grad, dst=0)
        if rank == 0:
            ok = ok and bool((grad.flat == 15.0).all())
        grad2 = torch.full((7,), float(rank + 1))
        MV.reduce_gradients(grad2, all_ranks=True)
        ok = ok and bool((grad2 == 3.0).all())
        q.put((rank, ok, mine))
    finally:
        dist.destroy_process_group()


def test_launch_local_ranks_gloo():
    """bench.py --gpus N without an external launcher (gs_livm_amd.multiview.launch_local_ranks): N children with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set rendezvous over gloo, rank 0's line is relayed, status 0."""
    import io
    import json
    import sys
    child = ("import os, json, torch, torch.distributed as dist\n"
             "dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))\n"
             "assert os.environ['MASTER_ADDR'] == '127.0.0.1' and os.environ['LOCAL_RANK'] == os.environ['RANK']\n"
             "t = torch.tensor([float(os.environ['RANK']) + 1.0]); dist.all_reduce(t)\n"
             "if dist.get_rank() == 0: print(json.dumps({'n_gpus': dist.get_world_size(), 'sum': float(t)}))\n"
             "dist.destroy_process_group()\n")
    buf = io.StringIO()
    assert MV.launch_local_ranks([sys.executable, "-c", child], 3, out=buf, timeout=120) == 0
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(line) == 1 and json.loads(line[0]) == {"n_gpus": 3, "sum": 6.0}


def test_launch_local_ranks_reports_a_failed_rank():
    """a rank that dies takes the job down with a non-zero status instead of leaving its peers waiting."""
    import io
    import sys
    import time
    bad = "import os, sys, time\nif os.environ['RANK'] == '1': sys.exit(3)\ntime.sleep(60)\n"
    t0 = time.time()
    rc = MV.launch_local_ranks([sys.executable, "-c", bad], 2, out=io.StringIO(), err=io.StringIO(), timeout=120)
    assert rc == 3 and time.time() - t0 < 30


def test_launch_local_ranks_drains_the_pipes_while_the_ranks_run():
    """A rank that writes far more than a pipe buffer (64 KB) to stdout and stderr -- RCCL debug output, a long JSON
    line -- must not block on a parent that reads only when everyone has exited; and a rank that never ends is
    killed at the timeout (status 124)."""
    import io
    import sys
    import time
    chatty = ("import os, sys\n"
              "sys.stderr.write('e' * 300000 + '\\n'); sys.stderr.flush()\n"
              "if os.environ['RANK'] == '0': sys.stdout.write('{\"pad\": \"' + 'x' * 400000 + '\"}\\n')\n")
    out, err = io.StringIO(), io.StringIO()
    t0 = time.time()
    assert MV.launch_local_ranks([sys.executable, "-c", chatty], 2, out=out, err=err, timeout=60) == 0
    assert time.time() - t0 < 30 and len(out.getvalue()) > 400000 and err.getvalue().count("e") >= 600000
    t0 = time.time()
    rc = MV.launch_local_ranks([sys.executable, "-c", "import time\ntime.sleep(60)\n"], 2, out=io.StringIO(),
                               err=io.StringIO(), timeout=2)
    assert rc == 124 and time.time() - t0 < 30


def test_bench_refuses_a_rank_count_it_cannot_run():
    """python bench.py --gpus 2 on a host with fewer GPUs must fail loudly (never bench one GPU under n_gpus = 2)."""
    import subprocess
    import sys
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a host with fewer than 2 GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr and not r.stdout.strip()


def test_exchange_steps_world_size_2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = sorted(q.get(timeout=120) for _ in ps)
    [p.join(60) for p in ps]
    assert all(p.exitcode == 0 for p in ps)
    assert res[0][1] and res[1][1]
    assert res[0][2] == [0, 2, 4] and res[1][2] == [1, 3]


def test_view_threads_keeps_call_order_and_reraises():
    """gs_livm_amd.multiview.ViewThreads without a GPU kernel in sight: results come back in call order whatever thread
    ran them, and an exception in a worker is re-raised in the calling thread."""
    if not torch.cuda.is_available():
        pytest.skip("ViewThreads creates HIP streams")
    vt = MV.ViewThreads(3, "cuda:0")
    try:
        assert vt.render([lambda k=k: k * k for k in range(10)]) == [k * k for k in range(10)]
        with pytest.raises(ZeroDivisionError):
            vt.render([lambda: 1, lambda: 1 / 0, lambda: 3])
        assert vt.render([lambda: "still alive"]) == ["still alive"]
    finally:
        vt.close()
