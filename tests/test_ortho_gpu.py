"""The orthophoto kernels (csrc/ortho.hip) and the orthophoto stage of the pipeline on the GPU: keys, ids and RGBA bit-equal to
the numpy brute force of tests/test_ortho.py on random scenes, independence of batching and order, a textured scene, the full
2900 x 2900 raster, and the files written by predict_and_fuse(ortho=...), by two ranks, by predict --fuse --dsm --ortho and by
python -m deep3d_aerial_amd.ortho."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import pipeline_scene as PS
import test_ortho as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _views(vs):
    from deep3d_aerial_amd import ortho

    return [ortho.OrthoView(v["id"], v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["image"]).cuda())
            for v in vs]


def _run(height, grid, vs, tol=0.01, views_per_batch=None):
    from deep3d_aerial_amd import ortho

    rgba, view, key = ortho.dsm_to_ortho(torch.from_numpy(np.ascontiguousarray(height, np.float32)).cuda(), grid, _views(vs), tol,
                                         views_per_batch=views_per_batch)
    return key.cpu().numpy(), view.cpu().numpy(), rgba.cpu().numpy()


def _random_scene(seed):
    """Random DSM over ground + boxes with NaN cells and cells above the cameras' plane, views of different sizes (some partly
    off the raster, some tilted), depth maps perturbed around the truth with holes (0 and NaN)."""
    from deep3d_aerial_amd import dsm

    rng = np.random.default_rng(seed)
    grid = dsm.DsmGrid([-40.0, 40.0, -20.0, 20.0], [0.5, 0.4])
    boxes = [(-5.0, 5.0, -6.0, 6.0, 80.0), (12.0, 20.0, 2.0, 9.0, 88.0)]
    h = T.dsm_of(grid, boxes) + rng.uniform(-0.3, 0.3, grid.shape).astype(np.float32)
    h[rng.uniform(size=grid.shape) < 0.05] = np.nan
    h[rng.uniform(size=grid.shape) < 0.01] = -3.0   # below the cameras (z 0 .. 2): behind them
    vs = []
    for k in range(9):
        w, hh = int(rng.integers(60, 200)), int(rng.integers(50, 150))
        C = (rng.uniform(-70, 70), rng.uniform(-35, 35), rng.uniform(0.0, 2.0))
        tilt = (0.0, 0.0) if k % 3 == 0 else (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
        v = T.view(int(rng.integers(0, 1 << 30)), C, boxes, w=w, h=hh, f=rng.uniform(60, 140), tilt=tilt)
        d = v["depth"] * rng.uniform(0.985, 1.015, v["depth"].shape).astype(np.float32)
        d[rng.uniform(size=d.shape) < 0.03] = 0.0
        d[rng.uniform(size=d.shape) < 0.01] = np.nan
        v["depth"] = d.astype(np.float32)
        vs.append(v)
    vs.append(dict(vs[0], id=vs[0]["id"] ^ 1))   # a twin: exact ties
    return h, grid, vs


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("tol", [0.0, 0.01, 0.05])
def test_bit_equal_to_numpy_on_random_scenes(seed, tol):
    h, grid, vs = _random_scene(seed)
    key, view, rgba = _run(h, grid, vs, tol)
    wk, wv, wr = T.ortho_numpy(h, grid, vs, tol)
    assert np.array_equal(key, wk)
    assert np.array_equal(view, wv)
    assert np.array_equal(rgba, wr)
    n = (view >= 0).sum()
    assert 0.3 * view.size < n < view.size   # most cells seen, some not


def test_batching_order_and_culling_do_not_change_the_bits():
    h, grid, vs = _random_scene(7)
    ref = _run(h, grid, vs)
    rng = np.random.default_rng(0)
    for vpb in (1, 2, 3, 64):
        order = list(rng.permutation(len(vs)))
        got = _run(h, grid, [vs[i] for i in order], views_per_batch=vpb)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), vpb
    # culling only skips work: a tile with one cell per view, where the box is a point, against the brute force
    from deep3d_aerial_amd import dsm

    tiny = dsm.DsmGrid([-40.0, 40.0, -20.0, 20.0], [5.0, 5.0])   # 16 x 8: one tile
    ht = T.dsm_of(tiny, [T.BOX])
    for a, b in zip(_run(ht, tiny, vs), T.ortho_numpy(ht, tiny, vs)):
        assert np.array_equal(a, b)


def test_merging_keys_over_ranks_and_colouring_per_rank():
    """Two disjoint view sets selected separately, keys min-merged, each colouring its own winners into one raster: the result
    of one call over all views (what the pipeline does over ranks)."""
    from deep3d_aerial_amd import ortho

    h, grid, vs = _random_scene(3)
    ht = torch.from_numpy(h).cuda()
    va, vb = _views(vs[:4]), _views(vs[4:])
    ka = ortho.select_views(ht, grid, va)
    kb = ortho.select_views(ht, grid, vb)
    key = torch.minimum(ka, kb)
    rgba, view = ortho.colorize(key, ht, grid, va)
    rgba, view = ortho.colorize(key, ht, grid, vb, rgba, view)
    wk, wv, wr = T.ortho_numpy(h, grid, vs)
    assert np.array_equal(key.cpu().numpy(), wk) and np.array_equal(view.cpu().numpy(), wv) and np.array_equal(rgba.cpu().numpy(), wr)


def test_textured_scene_comes_back_as_its_texture():
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-40.0, 40.0, -20.0, 20.0], [0.25, 0.25])
    box = T.BOX
    west, east = T.view(1, (-60.0, 0.0, 0.0), [box]), T.view(2, (60.0, 0.0, 0.0), [box])
    nadir = T.view(3, (0.0, 30.0, 0.0), [box], tilt=(0.35, 0.0))
    key, view, rgba = _run(T.dsm_of(grid, [box]), grid, [west, east, nadir])
    X, Y = T._centres(grid)
    ground = (np.abs(X) > 6.0) | (np.abs(Y) > 7.0)
    seen = view >= 0
    tex = T.texture(X, Y)
    err = np.abs(rgba[..., :3].astype(float) - tex).max(-1)
    # away from the box within the bilinear error; beside its edges the taps can straddle the roof edge in the image (no
    # blending along those seams: out of scope)
    assert err[ground & seen & (np.abs(X) > 11)].max() <= 3.0
    assert (err[ground & seen] <= 3.0).mean() > 0.99
    # the ground east of the box is hidden from the west camera by the roof: never coloured from it (and vice versa)
    band = (np.abs(Y) < 4.0)
    assert (view[band & (X > 6.0) & (X < 20.0)] != 1).all()
    assert (view[band & (X < -6.0) & (X > -20.0)] != 2).all()
    roof = (np.abs(X) < 3.5) & (np.abs(Y) < 4.5)
    rt = T.texture(X + 50.0, Y - 30.0)
    assert np.abs(rgba[roof][:, :3].astype(float) - rt[roof]).max() <= 3.0


def test_full_size_raster_with_64_views_equals_a_batched_run():
    from deep3d_aerial_amd import ortho, synthetic as S

    h, grid, raw = S.make_ortho_scene(2900, 2900, 0.2, 64, 688, 464, seed=5)
    views = [ortho.OrthoView(*v) for v in raw]
    rgba, view, key = ortho.dsm_to_ortho(h, grid, views)
    rgba2, view2, key2 = ortho.dsm_to_ortho(h, grid, views[::-1], views_per_batch=13)
    assert torch.equal(key, key2) and torch.equal(view, view2) and torch.equal(rgba, rgba2)
    assert int((view >= 0).sum()) > 0.5 * grid.width * grid.height


def test_sizes_ids_and_devices_are_checked():
    from deep3d_aerial_amd import dsm, ortho

    d = torch.ones(4, 5, device="cuda")
    with pytest.raises(ValueError, match="differ in size"):
        ortho.OrthoView(0, np.eye(3), np.eye(4), d, torch.zeros(4, 6, 3, dtype=torch.uint8, device="cuda"))
    grey = ortho.OrthoView(0, np.eye(3), np.eye(4), d, torch.full((4, 5), 9, dtype=torch.uint8, device="cuda"))
    assert torch.equal(grey.rgba[0, 0].cpu(), torch.tensor([9, 9, 9, 255], dtype=torch.uint8))
    grid = dsm.DsmGrid([0.0, 4.0, 0.0, 4.0], [1.0, 1.0])
    with pytest.raises(ValueError, match="unique"):
        ortho.select_views(torch.zeros(4, 4, device="cuda"), grid, [grey, grey])
    with pytest.raises(ValueError, match="does not match the grid"):
        ortho.select_views(torch.zeros(4, 3, device="cuda"), grid, [grey])


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _border(tmp_path):
    from deep3d_aerial_amd import pipeline

    scene = PS.SceneViews()
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "probe"), checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False)
    xyz = torch.cat([r["points"]["xyz"] for r in res]).cpu().numpy()
    lo, hi = np.floor(xyz.min(0)) - 2, np.ceil(xyz.max(0)) + 2
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])], 0.5


def test_predict_and_fuse_writes_the_orthophoto_dsm_to_ortho_gives(tmp_path):
    import dsm_scene
    from deep3d_aerial_amd import dsm, ortho, pipeline

    border, unit = _border(tmp_path)
    scene = OS.ImageSceneViews()
    tm = {}
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "a" / "MVS"), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                              min_geo_consist_num=3, filter_sources=False, timings=tm,
                              dsm=dsm_scene.settings(str(tmp_path / "a" / "dsm.tif"), border, unit),
                              ortho=OS.ortho_settings(str(tmp_path / "a" / "ortho.tif")))
    assert tm["ortho_s"] > 0
    h, grid = dsm.read_dsm(str(tmp_path / "a" / "dsm.tif"))
    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(ortho.OrthoView(int(it["outlocation"][2]), it["outcam"][1, :3, :3], it["outcam"][0],
                                     torch.from_numpy(scene.views[i]["depth"]).cuda(), torch.from_numpy(it["outimage"]).cuda()))
    rgba, view, _ = ortho.dsm_to_ortho(torch.from_numpy(h).cuda(), grid, views)
    ortho.write_ortho(str(tmp_path / "b.tif"), rgba, grid)
    assert (tmp_path / "a" / "ortho.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    assert (tmp_path / "a" / "ortho.tfw").read_text() == (tmp_path / "a" / "dsm.tfw").read_text()
    assert int((view >= 0).sum()) > 1000
    # the texture comes back where the DSM is close to the plane the views saw
    from PIL import Image

    assert Image.open(str(tmp_path / "a" / "ortho.tif")).mode == "RGBA"


def _launch(n_ranks, out_dir, border, unit):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "ortho_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(unit)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_orthophoto_one_rank_writes(tmp_path):
    border, unit = _border(tmp_path)
    out1 = _launch(1, tmp_path / "one", border, unit)
    out2 = _launch(2, tmp_path / "two", border, unit)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    for f in ("ortho.tif", "ortho.tfw", "dsm.tif"):
        assert (tmp_path / "one" / f).read_bytes() == (tmp_path / "two" / f).read_bytes(), f
    from PIL import Image

    a = np.array(Image.open(str(tmp_path / "one" / "ortho.tif")))
    assert (a[..., 3] == 255).sum() > 1000


def test_predict_main_fuse_dsm_ortho_and_the_standalone_cli(tmp_path):
    """predict --fuse --dsm --ortho on the block fixture (seeded casmvsnet weights: plumbing, not geometry) and
    python -m deep3d_aerial_amd.ortho on the MVS folder predict wrote give the same file."""
    import block_fixture as BF
    from deep3d_aerial_amd import mvs_dl, predict as P, synthetic as S

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    S.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    dsm_s = {"path": str(tmp_path / "dsm" / "block.tif"), "border": [-5000.0, 5000.0, -5000.0, 5000.0], "unit": [10.0, 10.0],
             "size": None, "select": "Max", "min_points": 1, "interpolation": "MovingAverage", "radius": 3, "iterations": 2}
    ortho_s = {"path": str(tmp_path / "ortho" / "block.tif"), "depth_tolerance": 0.5, "views_per_batch": 2}
    mvs = tmp_path / "MVS"
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         dsm=dsm_s, ortho=ortho_s,
                         extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                     "--position_threshold=50"]).run(folder, str(mvs))
    tif = tmp_path / "ortho" / "block.tif"
    assert tif.exists()
    cli = tmp_path / "cli" / "block.tif"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.ortho", "--dsm", dsm_s["path"], "--mvs", str(mvs), "--out", str(cli),
                          "--depth_tolerance", "0.5"],
                         cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == tif.read_bytes()
    assert (tmp_path / "cli" / "block.tfw").read_bytes() == (tmp_path / "dsm" / "block.tfw").read_bytes()
