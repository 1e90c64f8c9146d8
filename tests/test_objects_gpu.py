"""The object segmentation on the GPU (csrc/objects.hip, deep3d_aerial_amd/objects.py) against the numpy restatement of
tests/objects_scene.py, bit for bit: the root raster of label_components over rasters on either side of every tile length and
patterns that wind through the tiles, segment (label and every table column) on the analytic scene, on one large component and
with the opening on, the C ABI's refusals, the files, the pipeline stage and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import objects_scene as S
import pipeline_scene as PS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64   # the tile side (D3D_OBJECTS_TILE; test_the_tile_side_is_the_one_the_shapes_straddle holds it)
SIDES = (T - 1, T, T + 1, 2 * T + 1)
SHAPES = [(1, 1), (1, 2 * T + 2), (2 * T + 2, 1)] + [(h, w) for h in SIDES for w in SIDES]


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def test_the_tile_side_is_the_one_the_shapes_straddle():
    from deep3d_aerial_amd import objects

    assert objects.TILE == T


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_label_components_equals_the_restatement(shape):
    from deep3d_aerial_amd import objects

    for name, m in S.patterns(*shape).items():
        d8, db = _cuda(m.astype(np.uint8)), _cuda(m)
        for conn in (4, 8):
            want = S.roots(m, conn)
            got = objects.label_components(d8, conn)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (name, conn)
            if name in ("random_0.59", "serpentine"):
                assert np.array_equal(objects.label_components(db, conn).cpu().numpy(), want), (name, conn, "bool")
        assert np.array_equal(d8.cpu().numpy(), m.astype(np.uint8))                    # the input is not written


@pytest.mark.parametrize("shape", [(3 * T - 2, 3 * T + 9), (2 * T + 5, 4 * T)], ids=lambda s: "%dx%d" % s)
def test_winding_components_over_three_by_three_tiles(shape):
    from deep3d_aerial_amd import objects

    H, W = shape
    cases = {k: v for k, v in S.patterns(H, W).items() if k in ("serpentine", "serpentine_columns", "u", "rings", "rings_diagonal", "comb", "random_0.59")}
    cases["u_turned"] = S.u_shape(H, W)[::-1, ::-1].copy()      # the arms meet in the first row: the root's own tile
    cases["serpentine_wide"] = S.serpentine(H, W, gap=3)
    for name, m in cases.items():
        for conn in (4, 8):
            info = {}
            got = objects.label_components(_cuda(m.astype(np.uint8)), conn, info=info)
            assert np.array_equal(got.cpu().numpy(), S.roots(m, conn)), (name, conn)
            assert info["hooks"] >= 0 and info["repeats"] >= 0
            if name == "serpentine":                             # one component: every tile's pieces were hooked together
                assert info["hooks"] >= 8 and set(np.unique(got.cpu().numpy())) == {-1, 0}


def _grid(sc):
    from deep3d_aerial_amd.dsm import DsmGrid

    H, W = sc["ndsm"].shape
    return DsmGrid(sc["border"], list(sc["unit"]), size=(W, H))


def _same(got, want):
    label, table = got
    return label.dtype == torch.int32 and np.array_equal(label.cpu().numpy(), want[0]) and S.same_table(table, want[1])


@pytest.fixture(scope="module", params=[(0.5, 0.5), (0.5, 0.25)], ids=["square", "tall"])
def scene_case(request):
    sc = S.scene(S.SMALL, unit=request.param)
    return sc, _grid(sc)


def test_segment_on_the_scene_equals_the_restatement(scene_case):
    from deep3d_aerial_amd import objects

    sc, grid = scene_case
    d = _cuda(sc["ndsm"])
    for params in (dict(), dict(connectivity=4), dict(min_area=2.0), dict(min_height=0.0, min_area=0.0), dict(min_height=6.5, min_area=1.0)):
        want = S.segment(sc["ndsm"], sc["unit"], sc["origin"], **params)
        got = objects.segment(d, grid, **params)
        assert _same(got, want), params
    want = S.segment(sc["ndsm"], sc["unit"], sc["origin"])
    assert 2 <= want[1]["id"].shape[0] < len(np.unique(S.roots(S.foreground(sc["ndsm"], sc["unit"])))) - 1      # kept and dropped ones
    # run to run, and the foreground on its own
    a, b = objects.segment(d, grid), objects.segment(d, grid)
    assert torch.equal(a[0], b[0]) and S.same_table(a[1], b[1])
    fg = objects.foreground(d, grid, 2.0)
    assert fg.dtype == torch.uint8 and np.array_equal(fg.cpu().numpy(), S.foreground(sc["ndsm"], sc["unit"], 2.0).astype(np.uint8))
    assert np.array_equal(d.cpu().numpy().view(np.uint32), sc["ndsm"].view(np.uint32))


def test_segment_with_the_opening_on(scene_case):
    from deep3d_aerial_amd import objects

    sc, grid = scene_case
    d = _cuda(sc["ndsm"])
    for open_ in (0.5, 1.0):
        want_fg = S.foreground(sc["ndsm"], sc["unit"], 2.0, open_)
        assert 0 < want_fg.sum() < S.foreground(sc["ndsm"], sc["unit"], 2.0).sum()
        assert np.array_equal(objects.foreground(d, grid, 2.0, open_).cpu().numpy(), want_fg.astype(np.uint8))
        want = S.segment(sc["ndsm"], sc["unit"], sc["origin"], min_area=1.0, open=open_)
        assert _same(objects.segment(d, grid, min_area=1.0, open=open_), want) and want[1]["id"].shape[0] >= 2
    with pytest.raises(ValueError, match="outside 1..1024"):
        objects.segment(d, grid, open=0.05)


def _big():
    """150 x 200: one component of more than 10^4 cells with holes and fractional heights, islands beside it, a saturating height."""
    rng = np.random.default_rng(5)
    h = (rng.integers(0, 4096, (150, 200)) / 256.0).astype(np.float32)          # 0 .. 16 in steps of 1/256: q rounds
    h[rng.random(h.shape) < 0.1] = np.nan
    h[:, 150:156] = 0.5                                                          # a ditch: the islands beyond it are their own
    h[40:44, 160:190] = 1.0
    h[100, 20] = 5.0e6                                                           # q saturates at 2^32 - 1
    h[3, 3] = np.float32(2.0) - np.float32(2.0 ** -22)                           # just below min_height
    h[4, 4] = 2.0
    return h


def test_segment_on_one_large_component():
    from deep3d_aerial_amd import objects
    from deep3d_aerial_amd.dsm import DsmGrid

    h = _big()
    grid = DsmGrid([-3.0, -3.0 + 200 * 0.25, 7.0, 7.0 + 150 * 0.5], [0.25, 0.5], size=(200, 150))
    origin = (-3.0, 7.0 + 150 * 0.5)
    for params in (dict(min_height=2.0, min_area=1.0), dict(min_height=2.0, min_area=1.0, connectivity=4), dict(min_height=0.0, min_area=0.0)):
        want = S.segment(h, (0.25, 0.5), origin, **params)
        info = {}
        got = objects.segment(_cuda(h), grid, info=info, **params)
        assert _same(got, want), params
        assert info["objects"] == want[1]["id"].shape[0] and info["components"] >= info["objects"]
    want = S.segment(h, (0.25, 0.5), origin, min_height=2.0, min_area=1.0)
    assert want[1]["cells"].max() > 10000 and want[1]["height_max"].max() == 5.0e6
    assert (want[1]["volume"] > 2.0 ** 32 / 1024.0 * 0.125).any()                 # the saturated cell is in the large one


def test_segment_on_a_comb_whose_teeth_are_one_cell_runs_of_one_id():
    """3 x 200, connectivity 4: row 0 is foreground in every other column, row 1 is full, row 2 is empty.  The statistics pass
    then sees, in each wave of row 0, up to 32 one-cell runs of the same id with background runs between them: equal ids that
    are not adjacent are separate runs, and each is sent on its own."""
    from deep3d_aerial_amd import objects
    from deep3d_aerial_amd.dsm import DsmGrid

    rng = np.random.default_rng(11)
    h = (rng.integers(512, 4096, (3, 200)) / 256.0).astype(np.float32)           # 2 .. 16 in steps of 1/256: all foreground
    h[0, 1::2] = 0.0
    h[2, :] = 0.0
    assert (h[0, 0::2] >= 2.0).all() and (h[1] >= 2.0).all()
    grid = DsmGrid([0.0, 200 * 0.5, 0.0, 3 * 0.5], [0.5, 0.5], size=(200, 3))
    want = S.segment(h, (0.5, 0.5), (0.0, 1.5), min_area=1.0, connectivity=4)
    assert want[1]["cells"].tolist() == [300] and want[1]["j0"].tolist() == [0] and want[1]["j1"].tolist() == [199]
    assert set(np.unique(want[0][0])) == {0, 1} and (want[0][1] == 1).all() and not want[0][2].any()
    assert _same(objects.segment(_cuda(h), grid, min_area=1.0, connectivity=4), want)


def test_empty_rasters():
    from deep3d_aerial_amd import objects
    from deep3d_aerial_amd.dsm import DsmGrid

    for shape in ((1, 1), (70, 131)):
        H, W = shape
        grid = DsmGrid([0.0, W * 1.0, 0.0, H * 1.0], [1.0, 1.0], size=(W, H))
        for h in (np.zeros(shape, np.float32), np.full(shape, np.nan, np.float32), np.full(shape, -np.inf, np.float32),
                  np.full(shape, np.inf, np.float32)):
            label, table = objects.segment(_cuda(h), grid)
            assert label.shape == shape and not label.any() and S.same_table(table, S.segment(h, (1.0, 1.0), (0.0, float(H)))[1])
            assert all(table[c].shape == (0,) for c in S.COLUMNS)
            assert (objects.label_components(_cuda(np.zeros(shape, np.uint8)), 8) == -1).all()
    one = objects.segment(_cuda(np.full((1, 1), 3.0, np.float32)), DsmGrid([0.0, 1.0, 0.0, 1.0], [1.0, 1.0], size=(1, 1)), min_area=1.0)
    assert one[0].tolist() == [[1]] and one[1]["cells"].tolist() == [1] and one[1]["volume"].tolist() == [3.0]


def test_the_abi_refuses_bad_arguments_before_any_launch():
    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    W, H = 40, 30
    a = torch.full((H, W), 3.0, device="cuda")
    f = torch.full((H, W), 7.0, device="cuda")
    m = torch.full((H, W), 5, dtype=torch.uint8, device="cuda")
    par = torch.full((H, W), 9, dtype=torch.int32, device="cuda")
    lab = torch.full((H, W), 9, dtype=torch.int32, device="cuda")
    acc = torch.full((4, 9), 9, dtype=torch.int64, device="cuda")
    fid = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), 9, dtype=torch.int64, device="cuda")
    need = lib.d3d_objects_scratch_bytes(W, H)
    assert need >= W * H * 4 and lib.d3d_objects_scratch_bytes(0, 4) == 0 and lib.d3d_objects_scratch_bytes(65536, 32768) == 0
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def refused(rc, word):
        assert rc == -1 == _lib.ERR_INVALID_ARG and word in lib.d3d_last_error(), (rc, lib.d3d_last_error())

    refused(lib.d3d_objects_foreground(None, 2.0, P(m), None, W, H, None), b"null")
    refused(lib.d3d_objects_foreground(P(a), 2.0, None, None, W, H, None), b"null")
    refused(lib.d3d_objects_foreground(P(a), 2.0, P(m), None, 0, H, None), b"raster")
    refused(lib.d3d_objects_foreground(P(a), float("nan"), P(m), None, W, H, None), b"NaN")
    refused(lib.d3d_objects_foreground(P(a), 2.0, None, P(a), W, H, None), b"alias")
    refused(lib.d3d_objects_label(P(a), 2.0, None, 8, None, W, H, None, None), b"null")
    refused(lib.d3d_objects_label(None, 2.0, None, 8, P(par), W, H, None, None), b"exactly one")
    refused(lib.d3d_objects_label(P(a), 2.0, P(m), 8, P(par), W, H, None, None), b"exactly one")
    for conn in (0, 6, -8, 9):
        refused(lib.d3d_objects_label(P(a), 2.0, None, conn, P(par), W, H, None, None), b"connectivity")
    refused(lib.d3d_objects_label(P(a), float("nan"), None, 8, P(par), W, H, None, None), b"NaN")
    refused(lib.d3d_objects_label(P(a), 2.0, None, 8, P(par), 65536, 32768, None, None), b"2^31")
    refused(lib.d3d_objects_label(P(a), 2.0, None, 8, P(par), (1 << 31) - 1, 1, None, None), b"2^31")
    refused(lib.d3d_objects_label(P(a), 2.0, None, 8, P(a), W, H, None, None), b"alias")
    refused(lib.d3d_objects_roots(None, W, H, P(scratch), need, P(cnt), None), b"null")
    refused(lib.d3d_objects_roots(P(par), W, H, P(scratch), need, None, None), b"null")
    refused(lib.d3d_objects_roots(P(par), W, H, P(scratch), need - 1, P(cnt), None), b"scratch")
    refused(lib.d3d_objects_roots(P(par), W, -1, P(scratch), need, P(cnt), None), b"raster")
    refused(lib.d3d_objects_roots(P(par), W, H, P(par), need, P(cnt), None), b"alias")
    refused(lib.d3d_objects_stats(P(a), P(par), W, H, P(scratch), need, 4, None, None), b"null")
    refused(lib.d3d_objects_stats(P(a), P(par), W, H, P(scratch), need - 1, 4, P(acc), None), b"scratch")
    refused(lib.d3d_objects_stats(P(a), P(par), W, H, P(scratch), need, -1, P(acc), None), b"n_roots")
    refused(lib.d3d_objects_stats(P(a), P(par), W, H, P(scratch), need, W * H + 1, P(acc), None), b"n_roots")
    refused(lib.d3d_objects_relabel(P(par), P(acc), 4, 1, P(fid), None, W, H, P(scratch), need, P(cnt), None), b"null")
    refused(lib.d3d_objects_relabel(P(par), P(acc), 4, 0, P(fid), P(lab), W, H, P(scratch), need, P(cnt), None), b"min_cells")
    refused(lib.d3d_objects_relabel(P(par), P(acc), -2, 1, P(fid), P(lab), W, H, P(scratch), need, P(cnt), None), b"n_roots")
    refused(lib.d3d_objects_relabel(P(par), P(acc), 4, 1, P(fid), P(lab), W, H, P(scratch), need - 1, P(cnt), None), b"scratch")
    refused(lib.d3d_objects_relabel(P(par), P(acc), 4, 1, P(fid), P(par), W, H, P(scratch), need, P(cnt), None), b"alias")
    torch.cuda.synchronize()
    # nothing was launched: no buffer changed
    assert bool((a == 3.0).all()) and bool((f == 7.0).all()) and bool((m == 5).all()) and bool((par == 9).all()) and bool((lab == 9).all())
    assert bool((acc == 9).all()) and bool((fid == 9).all()) and bool((cnt == 9).all()) and bool((scratch == 0).all())


def test_files_round_trip_and_the_cli(tmp_path):
    from deep3d_aerial_amd import objects
    from deep3d_aerial_amd.dsm import read_dsm, write_dsm

    sc = S.scene(S.SMALL)
    grid = _grid(sc)
    params = dict(min_height=2.0, min_area=5.0, connectivity=4, open=0.0)
    s = dict(params, path=str(tmp_path / "sub" / "o.tif"), table=str(tmp_path / "sub2" / "o.csv"), nodata=-7.0)
    label, table = objects.build_and_write(_cuda(sc["ndsm"]), grid, s)
    want_label, want_table = S.segment(sc["ndsm"], sc["unit"], sc["origin"], **params)
    assert np.array_equal(label.cpu().numpy(), want_label) and S.same_table(table, want_table) and want_table["id"].shape[0] >= 3
    back, g = read_dsm(s["path"])
    want_raster = np.where(np.isnan(sc["ndsm"]), np.float32(np.nan), want_label.astype(np.float32)).astype(np.float32)
    assert g == grid and np.array_equal(back.view(np.uint32), want_raster.view(np.uint32)) and np.isnan(back).sum() == sc["hole"].sum()
    assert open(s["path"][:-4] + ".tfw").read() == grid.tfw_text()
    assert open(s["table"], "rb").read() == S.csv_text(want_table).encode("ascii")
    only = objects.build_and_write(sc["ndsm"], grid, dict(params, path=str(tmp_path / "only" / "o.tif")))   # a host array; no table
    assert sorted(os.listdir(tmp_path / "only")) == ["o.tfw", "o.tif"] and torch.equal(only[0], label)
    # the CLI on the nDSM this project wrote
    write_dsm(str(tmp_path / "ndsm.tif"), sc["ndsm"], grid, nodata=-7.0)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.objects", "--ndsm", str(tmp_path / "ndsm.tif"), "--out", str(tmp_path / "cli" / "o.tif"),
           "--table", str(tmp_path / "cli" / "o.csv"), "--min_area", "5", "--connectivity", "4", "--nodata", "-7"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "objects" in res.stdout, (res.stdout[-2000:], res.stderr[-3000:])
    assert (tmp_path / "cli" / "o.tif").read_bytes() == open(s["path"], "rb").read()
    assert (tmp_path / "cli" / "o.csv").read_bytes() == open(s["table"], "rb").read()


def test_predict_and_fuse_writes_the_objects_and_leaves_the_dtm_alone(tmp_path):
    from deep3d_aerial_amd import dsm, pipeline
    import dsm_scene

    scene = PS.SceneViews()
    run = lambda out, **kw: pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / out / "MVS"), checker=PS.checker(),
                                                      fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True, **kw)
    xyz = torch.cat([r["points"]["xyz"] for r in run("probe")]).cpu().numpy()
    lo, hi = np.floor(xyz.min(0)) - 2, np.ceil(xyz.max(0)) + 2
    border, unit = [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])], 0.5
    terrain = lambda d: {"path": str(tmp_path / d / "dtm.tif"), "ndsm": str(tmp_path / d / "ndsm.tif"), "ground": str(tmp_path / d / "level.tif"),
                         "max_window": 8.5}
    # the scene is one tilted plane: its nDSM is 0 on the ground cells, so min_height 0 makes them the foreground
    params = dict(min_height=0.0, min_area=1.0, connectivity=8, open=0.0)
    plain_tm, tm = {}, {}
    run("a", dsm=dsm_scene.settings(str(tmp_path / "a" / "dsm.tif"), border, unit), dtm=terrain("a"), objects=None, timings=plain_tm)
    o = dict(params, path=str(tmp_path / "b" / "objects.tif"), table=str(tmp_path / "b" / "objects.csv"))
    run("b", dsm=dsm_scene.settings(str(tmp_path / "b" / "dsm.tif"), border, unit), dtm=terrain("b"), objects=o, timings=tm)
    assert "objects_s" not in plain_tm and tm["objects_s"] > 0 and tm["dtm_s"] > 0
    names = ["dsm.tfw", "dsm.tif", "dtm.tfw", "dtm.tif", "level.tfw", "level.tif", "ndsm.tfw", "ndsm.tif"]
    assert sorted(f for f in os.listdir(tmp_path / "a") if f != "MVS") == names
    for name in names:                                                              # with objects=None every file keeps its bytes
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    ndsm, grid = dsm.read_dsm(str(tmp_path / "b" / "ndsm.tif"))
    origin = (grid.x_min, grid.y_max)
    want_label, want_table = S.segment(ndsm, grid.unit, origin, **params)
    assert want_table["id"].shape[0] >= 1
    back, g = dsm.read_dsm(o["path"])
    want_raster = np.where(np.isnan(ndsm), np.float32(np.nan), want_label.astype(np.float32)).astype(np.float32)
    assert g == grid and np.array_equal(back.view(np.uint32), want_raster.view(np.uint32))
    assert open(o["table"], "rb").read() == S.csv_text(want_table).encode("ascii")
    # the mesh as the DSM's source takes the same step, on the nDSM of the raster the mesh rasteriser returned
    import dsm_mesh_scene as DMS
    import mesh_scene as MS

    border6, voxel, tm = border + [float(lo[2]), float(hi[2])], float((hi - lo).max()) / 96, {}
    o = dict(params, path=str(tmp_path / "c" / "objects.tif"))
    run("c", mesh=MS.pipeline_settings(str(tmp_path / "c" / "mesh.ply"), border6, voxel),
        dsm=DMS.settings(str(tmp_path / "c" / "dsm.tif"), border6, voxel),
        dtm={"path": str(tmp_path / "c" / "dtm.tif"), "ndsm": str(tmp_path / "c" / "ndsm.tif"), "max_window": 8.5}, objects=o, timings=tm)
    assert tm["objects_s"] > 0 and tm["mesh_s"] > 0
    ndsm, grid = dsm.read_dsm(str(tmp_path / "c" / "ndsm.tif"))
    want_label, _ = S.segment(ndsm, grid.unit, (grid.x_min, grid.y_max), **params)
    back, g = dsm.read_dsm(o["path"])
    assert g == grid and np.array_equal(back.view(np.uint32), np.where(np.isnan(ndsm), np.float32(np.nan), want_label.astype(np.float32)).view(np.uint32))
    assert sorted(f for f in os.listdir(tmp_path / "c") if f.endswith(".tif")) == ["dsm.tif", "dtm.tif", "ndsm.tif", "objects.tif"]
