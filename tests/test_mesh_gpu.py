"""The mesh kernels (csrc/mesh.hip) and the mesh stage of the pipeline on the GPU: brick list, per-voxel sum and count, vertices
and triangles bit-equal to the numpy restatement of tests/test_mesh.py on every scene of tests/mesh_scene.py, independence of the
batching, and the PLY written by predict_and_fuse(mesh=...) over one and two ranks, by predict --fuse --mesh and by
python -m deep3d_aerial_amd.mesh."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_scene as MS
import pipeline_scene as PS
import test_mesh as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _views(vs):
    from deep3d_aerial_amd import mesh

    return [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda()) for v in vs]


def _gpu(views, grid, views_per_batch=None, **kw):
    from deep3d_aerial_amd import mesh

    vol = mesh.tsdf_volume(_views(views), grid, views_per_batch=views_per_batch, **kw)
    V, F = mesh.extract(vol, grid)
    out = {k: vol[k].cpu().numpy() for k in ("bricks", "sum", "count")}
    out.update(vertices=V.cpu().numpy(), faces=F.cpu().numpy(), brick_index=vol["brick_index"].cpu().numpy())
    return out


def _same(got, want):
    assert np.array_equal(got["bricks"], want["bricks"])
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["sum"].view(np.int32), want["sum"].view(np.int32))
    assert got["vertices"].shape == want["vertices"].shape and np.array_equal(got["vertices"].view(np.int32), want["vertices"].view(np.int32))
    assert np.array_equal(got["faces"], want["faces"])


@pytest.mark.parametrize("name", ["plane", "boxes", "sphere"])
def test_bit_equal_to_numpy(name):
    from deep3d_aerial_amd import mesh

    border, voxel, views, _ = MS.SCENES[name]()
    grid = mesh.MeshGrid(border, voxel)
    got = _gpu(views, grid)
    want = T.mesh_numpy(views, grid)
    _same(got, want)
    idx = got["brick_index"].ravel()
    assert np.array_equal(np.flatnonzero(idx >= 0), want["bricks"]) and np.array_equal(idx[want["bricks"]], np.arange(len(want["bricks"])))
    assert len(want["faces"]) > 200


def test_grid_not_a_multiple_of_8_and_other_settings():
    from deep3d_aerial_amd import mesh

    border, voxel, views, _ = MS.plane_scene(seed=3, w=96, h=72)
    grid = mesh.MeshGrid([-7.3, 6.1, -5.9, 7.7, -0.7, 4.9], 0.3)
    assert all(n % 8 for n in grid.n)
    for kw in ({}, {"trunc": 0.5, "conf_threshold": 0.5}, {"trunc": 2.4, "conf_threshold": 0.0}):
        got = _gpu(views, grid, **kw)
        vol = T.integrate(views, grid, T.allocate(views, grid, kw.get("conf_threshold", 0.2)), kw.get("trunc"),
                          kw.get("conf_threshold", 0.2))
        want = {"bricks": T.allocate(views, grid, kw.get("conf_threshold", 0.2)), "sum": vol[0], "count": vol[1]}
        V, F = T.extract(grid, want["bricks"], vol[0], vol[1])
        want.update(vertices=V, faces=F)
        _same(got, want)


def test_batching_does_not_change_the_bits():
    from deep3d_aerial_amd import mesh

    border, voxel, views, _ = MS.boxes_scene()
    grid = mesh.MeshGrid(border, voxel)
    ref = _gpu(views, grid)
    for vpb in (1, 3, len(views)):
        _same(_gpu(views, grid, views_per_batch=vpb), ref)
    V, F = mesh.depth_to_mesh(_views(views), grid, views_per_batch=3)
    assert np.array_equal(V.cpu().numpy(), ref["vertices"]) and np.array_equal(F.cpu().numpy(), ref["faces"])


def test_empty_views_and_cpu_tensors():
    from deep3d_aerial_amd import mesh

    border, voxel, views, _ = MS.plane_scene()
    grid = mesh.MeshGrid(border, voxel)
    blind = [dict(views[0], depth=np.zeros_like(views[0]["depth"]))]
    V, F = mesh.depth_to_mesh(_views(blind), grid)
    assert V.shape == (0, 3) and F.shape == (0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.MeshView(views[0]["K"], views[0]["E"], torch.from_numpy(views[0]["depth"]), torch.from_numpy(views[0]["confidence"]))


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _border(tmp_path):
    from deep3d_aerial_amd import pipeline

    scene = PS.SceneViews()
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "probe"), checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False)
    xyz = torch.cat([r["points"]["xyz"] for r in res]).cpu().numpy()
    lo, hi = np.floor(xyz.min(0)) - 1, np.ceil(xyz.max(0)) + 1
    span = float((hi - lo).max())
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2])], span / 96


def test_predict_and_fuse_writes_the_mesh_depth_to_mesh_gives(tmp_path):
    from deep3d_aerial_amd import mesh, pipeline

    border, voxel = _border(tmp_path)
    scene = PS.SceneViews()
    tm = {}
    path = str(tmp_path / "a" / "mesh.ply")
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "a" / "MVS"), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                              min_geo_consist_num=3, filter_sources=False, timings=tm, mesh=MS.pipeline_settings(path, border, voxel))
    assert tm["mesh_s"] > 0
    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(mesh.MeshView(it["outcam"][1, :3, :3], it["outcam"][0], torch.from_numpy(scene.views[i]["depth"]).cuda(),
                                   torch.from_numpy(scene.views[i]["confidence"]).cuda()))
    V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
    mesh.write_ply(str(tmp_path / "b.ply"), V, F)
    assert open(path, "rb").read() == (tmp_path / "b.ply").read_bytes()
    assert F.shape[0] > 100


def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mesh_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_mesh_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import mesh

    border, voxel = _border(tmp_path)
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    assert (tmp_path / "one" / "mesh.ply").read_bytes() == (tmp_path / "two" / "mesh.ply").read_bytes()
    V, F = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    assert len(F) > 100


def test_predict_main_fuse_mesh_and_the_standalone_cli(tmp_path):
    """predict --fuse --mesh on the block fixture (seeded casmvsnet weights: plumbing, not geometry) and
    python -m deep3d_aerial_amd.mesh on the MVS folder predict wrote give the same file."""
    import block_fixture as BF
    from deep3d_aerial_amd import mvs_dl, predict as P, synthetic as S

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    S.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    ply = tmp_path / "mesh" / "block.ply"
    flags = ["--border=-200,400,-200,200,-600,100", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    mvs = tmp_path / "MVS"
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                     "--position_threshold=50", "--mesh", str(ply)] + ["--mesh_" + f[2:] for f in flags]).run(folder, str(mvs))
    assert ply.exists()
    cli = tmp_path / "cli" / "block.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.mesh", "--mvs", str(mvs), "--out", str(cli)] + flags,
                         cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == ply.read_bytes()
    assert mesh_header_ok(ply)


def mesh_header_ok(path):
    from deep3d_aerial_amd import mesh

    V, F = mesh.read_ply(str(path))
    return V.dtype == np.float32 and F.dtype == np.int32
