"""The terrain filter on the GPU (csrc/dtm.hip, deep3d_aerial_amd/dtm.py) against the numpy restatement of tests/dtm_scene.py,
bit for bit: erosion, dilation and opening over rasters and radii that cross every chunk, step and segment boundary of the
kernels, the level loop, the pull-push pyramid and the nDSM on the analytic scene, the C ABI's refusals, the files, the pipeline
stage and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtm_scene as S
import pipeline_scene as PS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows x columns: single cells, single rows and columns, and rasters whose rows and columns cross the 64-cell steps of the row
# passes, the 256-column blocks and the 32-row chunks of the column passes
SHAPES = [(1, 1), (1, 300), (300, 1), (67, 131), (300, 70), (70, 300)]
# (rx, ry): beside the issue's, 15 / 16 (the 32-row column chunk is one segment of 31 or less than one of 33), 341 / 342 and 511 / 512
# (the 1024-cell row chunk is one segment of 1023 or 1025, or three of 341.67)
RADII = [(1, 1), (2, 3), (31, 1), (32, 32), (33, 64), (1, 1024), (1024, 1024), (15, 16), (16, 15), (511, 512), (512, 341)]


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _raster(shape, seed):
    """Heights on a quarter grid (ties), a fifth of the cells empty, an empty island, -0.0 beside +0.0."""
    rng = np.random.default_rng(seed)
    h = (rng.integers(-40, 41, shape) / 4.0).astype(np.float32)
    h[rng.random(shape) < 0.2] = np.nan
    H, W = shape
    if H > 40 and W > 40:
        h[10:31, 20:38] = np.nan
    h[h == 0] = np.where(rng.random(int((h == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return h


_RASTERS = {}


def _case(shape):
    if shape not in _RASTERS:
        _RASTERS[shape] = _raster(shape, 7 + shape[0])
        _RASTERS[shape].setflags(write=False)
    return _RASTERS[shape]


@pytest.mark.parametrize("radius", RADII, ids=lambda r: "r%dx%d" % r)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_erode_dilate_open_equal_the_restatement(shape, radius):
    from deep3d_aerial_amd import dtm

    h = _case(shape)
    rx, ry = radius
    d = _cuda(h)
    for got, want in ((dtm.erode(d, rx, ry), S.erode(h, rx, ry)), (dtm.dilate(d, rx, ry), S.dilate(h, rx, ry)),
                      (dtm.open_(d, rx, ry), S.open_(h, rx, ry))):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(d.cpu().numpy().view(np.uint32), h.view(np.uint32))          # the input is not written


@pytest.mark.parametrize("radius", [(1, 1), (3, 40), (1024, 2)], ids=lambda r: "r%dx%d" % r)
def test_special_rasters(radius):
    from deep3d_aerial_amd import dtm

    rx, ry = radius
    rng = np.random.default_rng(3)
    cases = {"all NaN": np.full((70, 131), np.nan, np.float32), "equal values": np.full((70, 131), 2.5, np.float32),
             "one value": np.full((70, 131), np.nan, np.float32), "signed zeros": np.where(rng.random((70, 131)) < 0.5, -0.0, 0.0).astype(np.float32),
             "infinities and payloads": _raster((70, 131), 5).copy(), "islands": np.full((131, 70), 1.0, np.float32)}
    cases["one value"][69, 0] = -3.0
    odd = cases["infinities and payloads"]
    odd[3, 3], odd[5, 100], odd[60, 7] = np.inf, -np.inf, np.float32(3.4e38)
    odd.view(np.uint32)[np.isnan(odd)] = 0xffc12345                                     # NaNs of another sign and payload
    cases["islands"][20:110, 10:60] = np.nan                                           # larger than the first two windows
    cases["islands"][50:60, 30:40] = -1.0
    for name, h in cases.items():
        d = _cuda(h)
        for fn, ref in ((dtm.erode, S.erode), (dtm.dilate, S.dilate), (dtm.open_, S.open_)):
            assert np.array_equal(fn(d, rx, ry).cpu().numpy().view(np.uint32), ref(h, rx, ry).view(np.uint32)), (name, fn.__name__)


def _params(sc):
    return dict(max_window=sc["max_window"], slope=0.3, dh0=0.3, dh_max=2.5)


@pytest.fixture(scope="module", params=[(0.5, 0.5), (0.5, 0.25), (0.2, 0.5)], ids=["square", "tall", "wide"])
def scene_case(request):
    from deep3d_aerial_amd.dsm import DsmGrid

    sc = S.scene(S.SMALL, unit=request.param)
    H, W = sc["height"].shape
    ux, uy = sc["unit"]
    grid = DsmGrid([10.0, 10.0 + W * ux, -5.0, -5.0 + H * uy], [ux, uy], size=(W, H))
    return sc, grid, S.dsm_to_dtm(sc["height"], sc["unit"], **_params(sc)), S.classify_ground(sc["height"], sc["unit"], **_params(sc))


def test_the_scene_equals_the_restatement(scene_case):
    from deep3d_aerial_amd import dtm

    sc, grid, (want_dtm, want_level, want_ndsm), (_, want_surface) = scene_case
    assert len(dtm.levels(grid, **_params(sc))) >= 4 and 0 < (want_level == 0).sum() < want_level.size
    assert set(np.unique(want_level)) >= {0, 1, 3, 4, 255}                                # several levels strike
    d = _cuda(sc["height"])
    level, surface = dtm.classify_ground(d, grid, **_params(sc))
    assert level.dtype == torch.uint8 and np.array_equal(level.cpu().numpy(), want_level)
    assert np.array_equal(surface.cpu().numpy().view(np.uint32), want_surface.view(np.uint32))
    ground = np.where(want_level == 0, sc["height"], np.float32(np.nan)).astype(np.float32)
    filled = dtm.fill_pull_push(_cuda(ground))
    assert np.array_equal(filled.cpu().numpy().view(np.uint32), want_dtm.view(np.uint32))
    got = dtm.dsm_to_dtm(d, grid, **_params(sc))
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want_dtm.view(np.uint32))
    assert np.array_equal(got[1].cpu().numpy(), want_level)
    assert np.array_equal(got[2].cpu().numpy().view(np.uint32), want_ndsm.view(np.uint32))
    # run to run
    again = dtm.dsm_to_dtm(d, grid, **_params(sc))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, again))


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 3), (129, 65)], ids=lambda s: "%dx%d" % s)
def test_pull_push_on_odd_sizes(shape):
    from deep3d_aerial_amd import dtm

    rng = np.random.default_rng(11)
    some = (rng.integers(-40, 41, shape) / 8.0).astype(np.float32)
    some[rng.random(shape) < 0.7] = np.nan
    some[shape[0] // 2, shape[1] // 2] = 1.25
    corner = np.full(shape, np.nan, np.float32)
    corner[shape[0] - 1, 0] = -7.5
    for h in (some, corner, np.full(shape, np.nan, np.float32), np.full(shape, 3.0, np.float32)):
        d = _cuda(h)
        got = dtm.fill_pull_push(d).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), S.fill_pull_push(h).view(np.uint32))
        assert np.array_equal(d.cpu().numpy().view(np.uint32), h.view(np.uint32))
    assert (dtm.fill_pull_push(_cuda(corner)).cpu().numpy() == -7.5).all()


def test_the_abi_refuses_bad_arguments_before_any_launch():
    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    W, H = 40, 30
    a, b = torch.full((H, W), 1.0, device="cuda"), torch.full((H, W), 2.0, device="cuda")
    level = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    need = lib.d3d_dtm_scratch_bytes(W, H)
    assert need >= 2 * W * H * 4 and lib.d3d_dtm_scratch_bytes(0, 4) == 0 and lib.d3d_dtm_scratch_bytes(65536, 32768) == 0
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    bad = -1

    def refused(rc, word):
        assert rc == bad == _lib.ERR_INVALID_ARG and word in lib.d3d_last_error(), (rc, lib.d3d_last_error())

    for fn in (lib.d3d_dtm_erode, lib.d3d_dtm_dilate, lib.d3d_dtm_open):
        refused(fn(None, P(b), W, H, 1, 1, P(scratch), need, None), b"null")
        refused(fn(P(a), None, W, H, 1, 1, P(scratch), need, None), b"null")
        refused(fn(P(a), P(b), W, H, 1, 1, None, need, None), b"null")
        refused(fn(P(a), P(b), 0, H, 1, 1, P(scratch), need, None), b"raster")
        refused(fn(P(a), P(b), 65536, 32768, 1, 1, P(scratch), need, None), b"2^31")
        for rx, ry in ((0, 1), (1, 0), (1025, 1), (1, 1025), (-1, 1)):
            refused(fn(P(a), P(b), W, H, rx, ry, P(scratch), need, None), b"radius")
        refused(fn(P(a), P(b), W, H, 1, 1, P(scratch), need - 1, None), b"scratch")
        refused(fn(P(a), P(a), W, H, 1, 1, P(scratch), need, None), b"alias")
        refused(fn(P(a), P(scratch), W, H, 1, 1, P(scratch), need, None), b"alias")
    for k in (0, 255, -3):
        refused(lib.d3d_dtm_classify(P(a), P(b), 0.5, k, P(level), W, H, None), b"outside 1..254")
    refused(lib.d3d_dtm_classify(None, P(b), 0.5, 1, P(level), W, H, None), b"null")
    refused(lib.d3d_dtm_classify(P(a), P(b), 0.5, 1, None, W, H, None), b"null")
    refused(lib.d3d_dtm_classify(P(a), P(b), float("nan"), 1, P(level), W, H, None), b"NaN")
    refused(lib.d3d_dtm_classify(P(a), P(b), 0.5, 1, P(level), W, 0, None), b"raster")
    refused(lib.d3d_dtm_ground(P(a), None, P(b), W, H, None), b"null")
    refused(lib.d3d_dtm_ndsm(P(a), P(b), None, W, H, None), b"null")
    refused(lib.d3d_dtm_pull(None, W, H, P(b), None), b"null")
    refused(lib.d3d_dtm_pull(P(a), 65536, 32768, P(b), None), b"2^31")
    refused(lib.d3d_dtm_pull(P(a), W, H, P(a), None), b"alias")
    refused(lib.d3d_dtm_push(P(a), None, W, H, None), b"null")
    refused(lib.d3d_dtm_push(P(a), P(b), W, -1, None), b"raster")
    refused(lib.d3d_dtm_push(P(a), P(a), W, H, None), b"alias")
    torch.cuda.synchronize()
    # nothing was launched: no buffer changed
    assert bool((a == 1.0).all()) and bool((b == 2.0).all()) and bool((level == 9).all()) and bool((scratch == 0).all())


def test_files_round_trip(tmp_path):
    from deep3d_aerial_amd import dtm
    from deep3d_aerial_amd.dsm import DsmGrid, read_dsm

    sc = S.scene(S.SMALL)
    H, W = sc["height"].shape
    grid = DsmGrid([100.0, 100.0 + W * 0.5, 50.0, 50.0 + H * 0.5], [0.5, 0.5], size=(W, H))
    s = dict(_params(sc), path=str(tmp_path / "t.tif"), ndsm=str(tmp_path / "sub" / "n.tif"), ground=str(tmp_path / "g.tif"), nodata=-7.0)
    got = dtm.build_and_write(_cuda(sc["height"]), grid, s)
    want_dtm, want_level, want_ndsm = S.dsm_to_dtm(sc["height"], sc["unit"], **_params(sc))
    for path, want in ((s["path"], want_dtm), (s["ndsm"], want_ndsm),
                       (s["ground"], np.where(want_level == 255, np.float32(np.nan), want_level.astype(np.float32)))):
        back, g = read_dsm(path)
        assert g == grid and np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32)), path
        assert open(path[:-4] + ".tfw").read() == grid.tfw_text()
    assert np.array_equal(got[1].cpu().numpy(), want_level)
    only = dtm.build_and_write(sc["height"], grid, dict(_params(sc), path=str(tmp_path / "only" / "t.tif")))   # a host array; no extras
    assert sorted(os.listdir(tmp_path / "only")) == ["t.tfw", "t.tif"] and torch.equal(only[0], got[0])
    # the CLI on the DSM this project wrote
    from deep3d_aerial_amd.dsm import write_dsm

    write_dsm(str(tmp_path / "dsm.tif"), sc["height"], grid)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.dtm", "--dsm", str(tmp_path / "dsm.tif"), "--out", str(tmp_path / "cli" / "t.tif"),
           "--ndsm", str(tmp_path / "cli" / "n.tif"), "--ground", str(tmp_path / "cli" / "g.tif"), "--max_window", repr(sc["max_window"]),
           "--nodata", "-7"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "DTM" in res.stdout, (res.stdout[-2000:], res.stderr[-3000:])
    for name, path in (("t.tif", s["path"]), ("n.tif", s["ndsm"]), ("g.tif", s["ground"])):
        assert (tmp_path / "cli" / name).read_bytes() == open(path, "rb").read(), name


def test_predict_and_fuse_writes_the_dtm_and_leaves_the_dsm_alone(tmp_path):
    from deep3d_aerial_amd import dsm, pipeline
    import dsm_scene

    scene = PS.SceneViews()
    run = lambda out, **kw: pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / out / "MVS"), checker=PS.checker(),
                                                      fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True, **kw)
    xyz = torch.cat([r["points"]["xyz"] for r in run("probe")]).cpu().numpy()
    lo, hi = np.floor(xyz.min(0)) - 2, np.ceil(xyz.max(0)) + 2
    border, unit = [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1])], 0.5
    plain_tm, tm = {}, {}
    run("a", dsm=dsm_scene.settings(str(tmp_path / "a" / "dsm.tif"), border, unit), timings=plain_tm)
    t = {"path": str(tmp_path / "b" / "dtm.tif"), "ndsm": str(tmp_path / "b" / "ndsm.tif"), "ground": str(tmp_path / "b" / "level.tif"),
         "max_window": 8.5}
    run("b", dsm=dsm_scene.settings(str(tmp_path / "b" / "dsm.tif"), border, unit), dtm=t, timings=tm)
    assert "dtm_s" not in plain_tm and tm["dtm_s"] > 0 and tm["dsm_s"] > 0
    for name in ("dsm.tif", "dsm.tfw"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    assert sorted(f for f in os.listdir(tmp_path / "a") if f != "MVS") == ["dsm.tfw", "dsm.tif"]
    height, grid = dsm.read_dsm(str(tmp_path / "b" / "dsm.tif"))
    assert np.isfinite(height).sum() > 1000
    want_dtm, want_level, want_ndsm = S.dsm_to_dtm(height, grid.unit, max_window=8.5, slope=0.3, dh0=0.3, dh_max=2.5)
    for key, want in (("path", want_dtm), ("ndsm", want_ndsm), ("ground", np.where(want_level == 255, np.float32(np.nan), want_level.astype(np.float32)))):
        back, g = dsm.read_dsm(t[key])
        assert g == grid and np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32)), key
    # the mesh as the DSM's source takes the same step, on the raster the mesh rasteriser returned
    import dsm_mesh_scene as DMS
    import mesh_scene as MS

    border6, voxel, tm = border + [float(lo[2]), float(hi[2])], float((hi - lo).max()) / 96, {}
    run("c", mesh=MS.pipeline_settings(str(tmp_path / "c" / "mesh.ply"), border6, voxel),
        dsm=DMS.settings(str(tmp_path / "c" / "dsm.tif"), border6, voxel), dtm={"path": str(tmp_path / "c" / "dtm.tif"), "max_window": 8.5},
        timings=tm)
    assert tm["dtm_s"] > 0 and tm["mesh_s"] > 0
    height, grid = dsm.read_dsm(str(tmp_path / "c" / "dsm.tif"))
    assert np.isfinite(height).sum() > 1000
    back, g = dsm.read_dsm(str(tmp_path / "c" / "dtm.tif"))
    want = S.dsm_to_dtm(height, grid.unit, max_window=8.5, slope=0.3, dh0=0.3, dh_max=2.5)[0]
    assert g == grid and np.array_equal(back.view(np.uint32), want.view(np.uint32))
    assert sorted(f for f in os.listdir(tmp_path / "c") if f.endswith(".tif")) == ["dsm.tif", "dtm.tif"]
