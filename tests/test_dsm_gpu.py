"""The DSM kernels (csrc/dsm.hip) and the DSM stage of the pipeline on the GPU: Max, Robust_Max and the counts bit-equal to the
numpy restatement of tests/test_dsm.py, determinism under any order or split of the points, the MovingAverage fill, the
roof-with-spikes semantics, the full 2900 x 2900 raster, and the files written by predict_and_fuse(dsm=...), by two ranks, by
predict --fuse --dsm and by python -m deep3d_aerial_amd.dsm."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pipeline_scene as PS
from test_dsm import dsm_numpy, fill_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(xyz, grid, select="Max", trim=0.1, min_points=1):
    from deep3d_aerial_amd import dsm

    h, c = dsm.points_to_dsm(_dev(xyz), grid, select=select, trim=trim, min_points=min_points)
    wh, wc = dsm_numpy(xyz, grid, select, trim, min_points)
    assert h.shape == grid.shape and h.dtype == torch.float32 and c.dtype == torch.int32
    assert np.array_equal(c.cpu().numpy(), wc)
    assert np.array_equal(_bits(h.cpu().numpy()), _bits(wh)), (select, trim, min_points)
    return h, c


def _cloud(n, grid, seed, spread=1.15):
    """Points over (and a little beyond) the grid, denser towards the north-west corner (cells of every size), heights in
    [-50, 50] with repeats: ties inside cells."""
    rng = np.random.default_rng(seed)
    x = grid.x_min + ((rng.uniform(0, 1, n) ** 2 * (spread + 0.05) - 0.05) * (grid.width * grid.unit[0]))
    y = grid.y_max - ((rng.uniform(0, 1, n) ** 2 * (spread + 0.05) - 0.05) * (grid.height * grid.unit[1]))
    z = np.round(rng.uniform(-50, 50, n), 1)
    return np.stack([x, y, z], 1).astype(np.float32)


CASES = [("Max", 0.1, 1), ("Robust_Max", 0.0, 1), ("Robust_Max", 0.1, 1), ("Robust_Max", 0.5, 1), ("Max", 0.1, 3),
         ("Robust_Max", 0.1, 4)]


@pytest.mark.parametrize("n", [0, 1, 1000, 1000000])
@pytest.mark.parametrize("select,trim,min_points", CASES)
def test_exact_against_numpy(n, select, trim, min_points):
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-20.0, 40.0, 3.0, 28.0], [0.5, 0.25])   # 120 x 100 (non-square, non-square cells)
    xyz = _cloud(n, grid, seed=n)
    h, c = _check(xyz, grid, select, trim, min_points)
    if n >= 1000:
        assert int(c.sum()) > n // 2
    if n == 1000000:
        assert int(c.max()) > 32 and int(c[c > 0].min()) <= 32   # cells on both selection paths
    if n == 0:
        assert torch.isnan(h).all() and int(c.sum()) == 0


def test_edges_outside_points_and_special_values():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-3.0, 5.0, -2.0, 4.0, -10.0, 10.0], [1.0, 0.5])   # 8 x 12
    pts = []
    for x in np.arange(-3.0, 5.01, 0.5):          # cell edges, Xmin and Xmax included
        for y in np.arange(-2.0, 4.01, 0.25):     # Ymin and Ymax included
            pts.append([x, y, x * y])
    pts += [[0.1, 0.1, -10.0], [0.1, 0.1, 10.0], [0.2, 0.1, -10.000001], [0.2, 0.1, 10.000001],   # on / past Zmin, Zmax
            [-3.5, 1.0, 1.0], [5.5, 1.0, 1.0], [1.0, -2.5, 1.0], [1.0, 4.5, 1.0], [-1e30, 1.0, 1.0], [1.0, 1e30, 1.0],
            [np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.nan], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0],
            [1.0, 1.0, np.inf], [1.0, 1.0, -np.inf],
            [2.3, 2.3, 0.0], [2.3, 2.3, -0.0], [2.4, 2.4, -0.0], [2.6, 2.6, -0.0], [2.6, 2.6, 0.0], [2.6, 2.6, -0.0],
            [-2.5, -1.9, -7.5], [-2.5, -1.9, -3.25]]
    xyz = np.array(pts, np.float32)
    for select, trim, mp in CASES:
        _check(xyz, grid, select, trim, mp)
    zero = np.array([[2.3, 2.3, 0.0], [2.3, 2.3, -0.0], [2.4, 2.4, -0.0], [-2.5, -1.9, -0.0], [-2.5, -1.9, -0.0]], np.float32)
    h, _ = _check(zero, grid, "Max")
    assert not np.signbit(h[3, 5].item()) and np.signbit(h[11, 0].item())   # +0.0 above -0.0
    h, _ = _check(zero, grid, "Robust_Max", 0.5)
    assert np.signbit(h[3, 5].item())


def test_one_hot_cell_next_to_single_point_cells():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([0.0, 300.0, 0.0, 200.0], [1.0, 1.0])   # 300 x 200
    rng = np.random.default_rng(3)
    hot = np.stack([np.full(200000, 150.5), np.full(200000, 100.5), rng.standard_normal(200000) * 10], 1)
    hot[:1000, 2] = 7.0   # ties
    ys, xs = np.mgrid[0:200, 0:300]
    single = np.stack([xs.ravel() + 0.5, 199.5 - ys.ravel(), rng.uniform(0, 9, xs.size)], 1)
    single = single[(xs.ravel() != 150) | (ys.ravel() != 99)]
    xyz = np.concatenate([single[: len(single) // 2], hot, single[len(single) // 2:]]).astype(np.float32)
    for select, trim, mp in CASES:
        _, c = _check(xyz, grid, select, trim, mp)
    assert int(c.max()) == 200000 and int((c == 1).sum()) == 300 * 200 - 1


def test_any_order_and_split_give_the_same_bits():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-20.0, 40.0, 3.0, 28.0], [0.5, 0.25])
    xyz = _cloud(300000, grid, seed=11, spread=0.3)   # dense: hundreds of points per cell
    perm = np.random.default_rng(12).permutation(len(xyz))
    chunks = np.array_split(xyz[perm], 7)
    for select in ("Max", "Robust_Max"):
        for interp in (None, "MovingAverage"):
            a = dsm.points_to_dsm(_dev(xyz), grid, select, interpolation=interp)
            b = dsm.points_to_dsm(_dev(xyz[perm]), grid, select, interpolation=interp)
            c = dsm.points_to_dsm(torch.cat([_dev(ch) for ch in chunks]), grid, select, interpolation=interp)
            for u in (b, c):
                assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(u[0].cpu().numpy()))
                assert torch.equal(a[1], u[1])


def test_moving_average_fill():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([0.0, 97.0, 0.0, 61.0], [1.0, 1.0])   # 97 x 61
    rng = np.random.default_rng(5)
    xyz = _cloud(4000, grid, seed=6, spread=1.0)
    xyz[:, 2] = rng.uniform(-30, 30, len(xyz)).astype(np.float32)
    keep = ~((xyz[:, 0] > 40) & (xyz[:, 0] < 60) & (xyz[:, 1] > 20) & (xyz[:, 1] < 40))   # a 20 x 20 hole
    xyz = xyz[keep]
    h0, _ = dsm.points_to_dsm(_dev(xyz), grid, "Robust_Max")
    base = h0.cpu().numpy()
    for r in (1, 2, 5, 16):
        got = dsm.points_to_dsm(_dev(xyz), grid, "Robust_Max", interpolation="MovingAverage", radius=r)[0].cpu().numpy()
        want = fill_numpy(base, r)
        assert np.array_equal(_bits(got), _bits(want)), r
        valid = ~np.isnan(base)
        assert np.array_equal(_bits(got[valid]), _bits(base[valid]))   # non-empty cells untouched
        if r <= 5:
            assert np.isnan(got[32, 52])   # the middle of the 20-cell hole is farther than r from any point
    two = dsm.points_to_dsm(_dev(xyz), grid, "Robust_Max", interpolation="MovingAverage", radius=2, iterations=2)[0]
    once = dsm.fill_moving_average(h0, 2)
    twice = dsm.fill_moving_average(once, 2)
    assert np.array_equal(_bits(two.cpu().numpy()), _bits(twice.cpu().numpy()))
    assert np.array_equal(_bits(twice.cpu().numpy()), _bits(fill_numpy(fill_numpy(base, 2), 2)))
    assert np.array_equal(_bits(h0.cpu().numpy()), _bits(base))   # the input raster is not changed
    assert np.isnan(dsm.fill_moving_average(_dev(np.full((5, 7), np.nan)), 3).cpu().numpy()).all()


def roof_with_spikes(grid, per_cell, seed):
    """A gabled roof over the whole grid, `per_cell` points in every cell, and in 1 % of the cells one point 30 m above the roof."""
    rng = np.random.default_rng(seed)
    cells = grid.width * grid.height
    ci = np.repeat(np.arange(cells), per_cell)
    x = grid.x_min + (ci % grid.width + rng.uniform(0.01, 0.99, ci.size)) * grid.unit[0]
    y = grid.y_max - (ci // grid.width + rng.uniform(0.01, 0.99, ci.size)) * grid.unit[1]
    cx = grid.x_min + grid.width * grid.unit[0] / 2
    z = 100.0 - 0.3 * np.abs(x - cx) + 0.01 * rng.standard_normal(ci.size)
    spiked = rng.choice(cells, max(1, cells // 100), replace=False)
    z[spiked * per_cell] += 30.0
    return np.stack([x, y, z], 1).astype(np.float32), spiked


def test_robust_max_removes_spikes_that_max_keeps():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([0.0, 40.0, 0.0, 30.0], [1.0, 1.0])
    xyz, spikes = roof_with_spikes(grid, 20, 9)
    hm, c = _check(xyz, grid, "Max")
    hr, _ = _check(xyz, grid, "Robust_Max", 0.1)
    assert int(c.min()) >= 10
    hm, hr = hm.cpu().numpy(), hr.cpu().numpy()
    jx = np.arange(grid.width) + 0.5
    roof = (100.0 - 0.3 * np.abs(jx - 20.0))[None, :]
    assert (hm > roof + 10).sum() == len(spikes)             # Max keeps every spike
    assert np.abs(hr - roof).max() < 0.6                     # Robust_Max returns the roof (within a cell's slope)


def test_full_size_raster():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-430.0, 150.0, -330.0, 250.0, 700.0, 900.0], [0.2, 0.2])
    assert grid.shape == (2900, 2900)
    rng = np.random.default_rng(21)
    n = 20000000
    x = rng.uniform(-440.0, 160.0, n)
    y = rng.uniform(-340.0, 260.0, n)
    z = 720.0 + 60.0 * np.sin(x / 40.0) * np.cos(y / 55.0) + np.where(rng.uniform(0, 1, n) < 0.01, 50.0, 0.0)
    xyz = np.stack([x, y, z], 1).astype(np.float32)
    del x, y, z
    for select in ("Max", "Robust_Max"):
        _check(xyz, grid, select, 0.1)


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _scene_border(tmp_path):
    """The in-process single-rank fused points of pipeline_scene, and a border / unit around them."""
    from deep3d_aerial_amd import pipeline

    scene = PS.SceneViews()
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "probe"), checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True)
    xyz = torch.cat([r["points"]["xyz"] for r in res]).cpu().numpy()
    assert len(xyz) > 2000
    lo, hi = np.floor(xyz.min(0)) - 2, np.ceil(xyz.max(0)) + 2
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])], 0.5


def test_predict_and_fuse_writes_the_dsm_of_the_fused_points(tmp_path):
    from deep3d_aerial_amd import dsm, pipeline
    import dsm_scene

    border, unit = _scene_border(tmp_path)
    s = dsm_scene.settings(str(tmp_path / "a" / "dsm.tif"), border, unit)
    scene = PS.SceneViews()
    tm = {}
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "a" / "MVS"), checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True, timings=tm, dsm=s)
    assert tm["dsm_s"] > 0
    grid = dsm.DsmGrid(border, [unit, unit])
    h, _ = dsm.points_to_dsm(torch.cat([r["points"]["xyz"] for r in res]), grid, "Robust_Max", 0.1, interpolation="MovingAverage")
    dsm.write_dsm(str(tmp_path / "b.tif"), h, grid)
    assert (tmp_path / "a" / "dsm.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    assert (tmp_path / "a" / "dsm.tfw").read_text() == grid.tfw_text()
    assert int(torch.isfinite(h).sum()) > 1000
    # dsm=None: nothing new is written, the results are today's
    plain = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "c" / "MVS"), checker=PS.checker(),
                                      fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True)
    assert not any(f.endswith((".tif", ".tfw")) for _, _, fs in os.walk(tmp_path / "c") for f in fs)
    for x, y in zip(res, plain):
        assert torch.equal(x["points"]["xyz"], y["points"]["xyz"])


def _launch(n_ranks, out_dir, filter_sources, fuse_partition, border, unit):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dsm_scene.py"), str(out_dir), str(int(filter_sources)), fuse_partition,
           ",".join(repr(b) for b in border), repr(unit)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


@pytest.mark.parametrize("fuse_partition,filter_sources", [("views", False), ("scene_blocks", True)])
def test_two_ranks_write_the_dsm_one_rank_writes(tmp_path, fuse_partition, filter_sources):
    from PIL import Image

    border, unit = _scene_border(tmp_path)
    out1 = _launch(1, tmp_path / "one", filter_sources, fuse_partition, border, unit)
    out2 = _launch(2, tmp_path / "two", filter_sources, fuse_partition, border, unit)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    for f in ("dsm.tif", "dsm.tfw"):
        assert (tmp_path / "one" / f).read_bytes() == (tmp_path / "two" / f).read_bytes(), f
    a = np.array(Image.open(str(tmp_path / "one" / "dsm.tif")))
    assert (a != -9999.0).sum() > 1000


def test_predict_main_fuse_dsm_and_the_standalone_cli(tmp_path):
    """predict --fuse --dsm on the block fixture (seeded casmvsnet weights: plumbing, not geometry) writes a DSM PIL reads; the
    standalone CLI on the saved fused folder writes the same bytes."""
    import block_fixture as BF
    from PIL import Image
    from deep3d_aerial_amd import mvs_dl, predict as P, synthetic as S

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    S.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    settings = {"path": str(tmp_path / "dsm" / "block.tif"), "border": [-5000.0, 5000.0, -5000.0, 5000.0], "unit": [10.0, 10.0],
                "size": None, "select": "Robust_Max", "trim": 0.2, "min_points": 1, "interpolation": "MovingAverage", "radius": 3,
                "iterations": 2, "nodata": -9999.0}
    mvs = tmp_path / "MVS"
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         dsm=settings, extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                                   "--position_threshold=50"]).run(folder, str(mvs))
    tif = tmp_path / "dsm" / "block.tif"
    im = Image.open(str(tif))
    assert im.mode == "F" and im.size == (1000, 1000)
    assert (tmp_path / "dsm" / "block.tfw").read_text() == "10.0\n0\n0\n-10.0\n-5000.0\n5000.0"
    cli = tmp_path / "cli" / "block.tif"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.dsm", "--fused", str(mvs / "fused"), "--out", str(cli),
                          "--border=-5000,5000,-5000,5000", "--unit", "10", "--select", "Robust_Max", "--trim", "0.2",
                          "--interpolation", "MovingAverage", "--radius", "3", "--iterations", "2"],
                         cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == tif.read_bytes()
    assert (tmp_path / "cli" / "block.tfw").read_bytes() == (tmp_path / "dsm" / "block.tfw").read_bytes()
