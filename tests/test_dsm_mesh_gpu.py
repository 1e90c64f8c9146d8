"""The DSM from a mesh on the GPU (csrc/dsm.hip dsm_tri_*, dsm.mesh_to_dsm): bit-equal to the numpy restatement of
tests/test_dsm_mesh.py on analytic meshes, random soups (small and big triangles, so both kernels run) and the meshes of
tests/mesh_scene.py; independence of the face order, the winding and the split; the MovingAverage fill; the full 2900 x 2900
raster; and the files of predict_and_fuse(mesh=..., dsm={"source": "mesh"}, ortho=...) over one and two ranks against
python -m deep3d_aerial_amd.dsm --mesh."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dsm_mesh_scene as DMS
import mesh_scene as MS
import test_dsm_mesh as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _gpu(V, F, grid, **kw):
    from deep3d_aerial_amd import dsm

    v = torch.from_numpy(np.ascontiguousarray(V, np.float32).reshape(-1, 3)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(F, np.int32).reshape(-1, 3)).cuda()
    return dsm.mesh_to_dsm(v, f, grid, **kw).cpu().numpy()


def _same(got, want):
    assert got.shape == want.shape and np.array_equal(T._bits(got), T._bits(want))


def _tmax(a, b):
    """Cellwise max in the IEEE total order, NaN = empty."""
    ka, kb = T.keys_of(a), T.keys_of(b)
    ka = np.where(np.isnan(a), 0, ka)
    kb = np.where(np.isnan(b), 0, kb)
    k = np.maximum(ka, kb)
    return np.where(k == 0, np.float32(np.nan), T.unkey(k)).astype(np.float32)


def _big_count(V, F, grid):
    _, _, box = T.triangles(V, F)
    j0, j1, i0, i1, ok = T.cell_ranges(box, grid)
    from deep3d_aerial_amd import dsm

    return int((ok & ((j1 - j0 + 1) * (i1 - i0 + 1) > dsm.DSM_TRI_SMALL)).sum())


def test_analytic_meshes_are_bit_equal_to_numpy():
    from deep3d_aerial_amd import dsm

    g = dsm.DsmGrid([0.0, 12.0, 0.0, 9.0], [0.25, 0.5])
    cases = [(T.quad(-1.0, 13.0, -2.0, 10.0, lambda x, y: 0.3 * x - 0.7 * y + 20.0), g),
             (T.box_building(), dsm.DsmGrid([0.0, 8.0, 0.0, 6.0], [1.0, 1.0])),
             (T.box_building(), dsm.DsmGrid([0.0, 8.0, 0.0, 6.0, -1.0, 5.0], [0.1, 0.1])),
             (T.height_field(24, 0), dsm.DsmGrid([0.0, 24.0, 0.0, 24.0], [1.0, 1.0])),
             (T.height_field(24, 1), dsm.DsmGrid([0.5, 23.5, 0.5, 23.5], [0.25, 0.25])),
             (T.height_field(40, 2, spacing=0.3, origin=-1.0), dsm.DsmGrid([-0.7, 10.0, -0.4, 10.0], [0.1, 0.13]))]
    for (V, F), grid in cases:
        want = T.mesh_dsm_numpy(V, F, grid)
        _same(_gpu(V, F, grid), want)
    V, F = T.height_field(24, 0)
    assert not np.isnan(_gpu(V, F, dsm.DsmGrid([0.0, 24.0, 0.0, 24.0], [1.0, 1.0]))).any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_soups_small_and_big_are_bit_equal_to_numpy(seed):
    from deep3d_aerial_amd import dsm

    g = T.grid_small()
    gz = dsm.DsmGrid([0.0, 20.0, 0.0, 15.0, 0.0, 8.0], [0.5, 0.5])
    small = T.soup(5000, seed)
    big = T.soup(300, 100 + seed, big=True)
    both = T.merge(small, big)
    for (V, F), grid in ((small, g), (big, g), (both, g), (both, gz)):
        want = T.mesh_dsm_numpy(V, F, grid)
        _same(_gpu(V, F, grid), want)
    assert _big_count(*big, g) > 150 and 0 < _big_count(*small, g) < 2500
    assert np.isfinite(T.mesh_dsm_numpy(*big, g)).mean() > 0.9


@pytest.mark.parametrize("name", ["plane", "boxes", "sphere"])
def test_meshes_of_the_mesh_scenes_are_bit_equal_to_numpy(name):
    from deep3d_aerial_amd import dsm, mesh

    border, voxel, views, _ = MS.SCENES[name]()
    grid = mesh.MeshGrid(border, voxel)
    mv = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda()) for v in views]
    V, F = mesh.depth_to_mesh(mv, grid)
    V, F = V.cpu().numpy(), F.cpu().numpy()
    assert len(F) > 200
    for unit in (voxel * 0.8, voxel * 2.5):
        g = dsm.DsmGrid(border[:4], [unit, unit])
        want = T.mesh_dsm_numpy(V, F, g)
        _same(_gpu(V, F, g), want)
        assert np.isfinite(want).sum() > 40


def test_order_winding_and_split_do_not_change_the_bits():
    g = T.grid_small()
    rng = np.random.default_rng(3)
    V, F = T.merge(T.soup(4000, 7), T.soup(200, 8, big=True), T.height_field(16, 3, spacing=1.1, origin=0.3))
    ref = _gpu(V, F, g)
    assert np.isfinite(ref).sum() > 500
    _same(_gpu(V, F[rng.permutation(len(F))], g), ref)
    _same(_gpu(V, F[:, ::-1], g), ref)
    _same(_gpu(V, F[:, [2, 0, 1]], g), ref)
    p = rng.permutation(len(V))
    _same(_gpu(V[p], np.argsort(p)[F].astype(np.int32), g), ref)
    cut = rng.permutation(len(F))
    parts = [F[cut[:1000]], F[cut[1000:3000]], F[cut[3000:]]]
    merged = _gpu(V, parts[0], g)
    for part in parts[1:]:
        merged = _tmax(merged, _gpu(V, part, g))
    _same(merged, ref)


def test_moving_average_fill_is_the_point_dsms():
    from deep3d_aerial_amd import dsm

    g = T.grid_small()
    V, F = T.soup(800, 11)
    raw = _gpu(V, F, g)
    assert np.isnan(raw).sum() > 50
    for radius, iterations in ((1, 1), (2, 3)):
        want = dsm.fill_moving_average(torch.from_numpy(raw).cuda(), radius, iterations).cpu().numpy()
        _same(_gpu(V, F, g, interpolation="MovingAverage", radius=radius, iterations=iterations), want)


def test_empty_meshes_bad_indices_and_cpu_tensors():
    from deep3d_aerial_amd import dsm

    g = T.grid_small()
    assert np.isnan(_gpu(np.zeros((0, 3)), np.zeros((0, 3)), g)).all()
    assert np.isnan(_gpu(np.zeros((5, 3)), np.zeros((0, 3)), g)).all()
    V, F = T.soup(10, 1)
    for bad in (np.array([[0, 1, 30]]), np.array([[-1, 0, 1]])):
        with pytest.raises(ValueError, match="outside"):
            _gpu(V, np.concatenate([F, bad]), g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsm.mesh_to_dsm(torch.from_numpy(V).cuda(), torch.from_numpy(F), g)


def test_full_size_raster():
    from deep3d_aerial_amd import dsm

    g = dsm.DsmGrid([-430.0, 150.0, -330.0, 250.0, 700.0, 900.0], [0.2, 0.2])   # the reference's config.yaml CREATEDSM: 2900 x 2900
    assert g.shape == (2900, 2900)
    spans = T.quad(-431.0, 151.0, -331.0, 251.0, lambda x, y: 800.0 + 0.05 * x - 0.02 * y)   # two triangles over the whole raster
    hf = T.height_field(60, 4, spacing=2.0, origin=-300.0)
    hf = (hf[0] + np.array([0, 0, 805.0], np.float32), hf[1])
    V, F = T.merge(spans, hf)
    got = _gpu(V, F, g)
    assert not np.isnan(got).any()
    _same(got, T.mesh_dsm_numpy(V, F, g))


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _border(tmp_path):
    import test_mesh_gpu

    return test_mesh_gpu._border(tmp_path)


def _dsm_cli(ply, out, border, unit, *extra):
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.dsm", "--mesh", str(ply), "--out", str(out),
           "--border=%s" % ",".join(repr(b) for b in border[:4]), "--unit=%r" % unit] + list(extra)
    res = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout


def test_predict_and_fuse_writes_the_mesh_dsm_the_cli_writes_and_drapes_the_orthophoto(tmp_path):
    import ortho_scene as OS
    from deep3d_aerial_amd import dsm, mesh, ortho

    border, voxel = _border(tmp_path)
    tm = {}
    out = tmp_path / "a"
    DMS.run(str(out), border, voxel, timings=tm)
    assert tm["mesh_s"] > 0 and tm["dsm_s"] > 0 and tm["ortho_s"] > 0
    _dsm_cli(out / "mesh.ply", tmp_path / "cli.tif", border, voxel)
    assert (out / "dsm.tif").read_bytes() == (tmp_path / "cli.tif").read_bytes()
    assert (out / "dsm.tfw").read_text() == (tmp_path / "cli.tfw").read_text()
    h, grid = dsm.read_dsm(str(out / "dsm.tif"))
    V, F = mesh.read_ply(str(out / "mesh.ply"))
    _same(h, T.mesh_dsm_numpy(V, F, grid))
    assert np.isfinite(h).sum() > 1000
    # the orthophoto on that DSM is what ortho.dsm_to_ortho makes of it
    scene = OS.ImageSceneViews()
    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(ortho.OrthoView(int(it["outlocation"][2]), it["outcam"][1, :3, :3], it["outcam"][0],
                                     torch.from_numpy(scene.views[i]["depth"]).cuda(), torch.from_numpy(it["outimage"]).cuda()))
    rgba, view, _ = ortho.dsm_to_ortho(torch.from_numpy(h).cuda(), grid, views)
    ortho.write_ortho(str(tmp_path / "b.tif"), rgba, grid)
    assert (out / "ortho.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    assert int((view >= 0).sum()) > 1000


def test_the_cli_fill_equals_the_operator(tmp_path):
    from deep3d_aerial_amd import dsm, mesh

    V, F = T.soup(600, 21)
    mesh.write_ply(str(tmp_path / "s.ply"), V, F)
    g = T.grid_small()
    _dsm_cli(tmp_path / "s.ply", tmp_path / "s.tif", g.border, 0.5, "--interpolation", "MovingAverage", "--radius", "3")
    h, grid = dsm.read_dsm(str(tmp_path / "s.tif"))
    assert grid == g
    _same(h, _gpu(V, F, g, interpolation="MovingAverage", radius=3))


def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dsm_mesh_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_mesh_dsm_one_rank_writes(tmp_path):
    border, voxel = _border(tmp_path)
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1 dsm" in out1 and "rank 0/2 dsm" in out2 and "rank 1/2 dsm -" in out2
    for f in ("dsm.tif", "dsm.tfw", "mesh.ply", "ortho.tif"):
        assert (tmp_path / "one" / f).read_bytes() == (tmp_path / "two" / f).read_bytes(), f
