"""CPU checks of the DSM stage (deep3d_aerial_amd/dsm.py, csrc/dsm.hip; the reference's CREATEDSM step, run.py:209-247, whose
pc2dsm module it never shipped): the grid and world file against the reference's gdal_create_dsm_file formulas, the TIFF
writer, the C ABI and its argument checks, the CLI flags and the config plumbing.  `dsm_numpy` / `fill_numpy` restate the
semantics in numpy; tests/test_dsm_gpu.py compares the kernels against them bit for bit."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from deep3d_aerial_amd import _lib, dsm, mvs_dl, predict

NEW_SYMBOLS = ("d3d_dsm_scratch_bytes", "d3d_dsm_from_points", "d3d_dsm_fill_moving_average")


# ----------------------------------------------------------------------------------------
# numpy restatement (fp64 cell index, ordered uint32 keys, per-cell sort)
# ----------------------------------------------------------------------------------------
def keys_of(z):
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def cells_of(xyz, grid):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z >= grid.z_min) & (z <= grid.z_max)
        fj = np.floor((x - grid.x_min) / grid.unit[0])
        fi = np.floor((grid.y_max - y) / grid.unit[1])
    keep &= (fj >= 0) & (fj < grid.width) & (fi >= 0) & (fi < grid.height)
    cell = np.where(keep, np.where(keep, fi, 0).astype(np.int64) * grid.width + np.where(keep, fj, 0).astype(np.int64), -1)
    return cell, keep


def dsm_numpy(xyz, grid, select="Max", trim=0.1, min_points=1):
    """(height [H,W] float32 with NaN, count [H,W] int32) as dsm.py's docstring states them."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cell, keep = cells_of(xyz, grid)
    c, k = cell[keep], keys_of(xyz[keep, 2])
    cells = grid.width * grid.height
    count = np.bincount(c, minlength=cells).astype(np.int64)
    order = np.lexsort((~k, c))              # by cell, then key descending
    ks = k[order]
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    t = np.floor(float(trim) * count.astype(np.float64)).astype(np.int64) if select == "Robust_Max" else np.zeros_like(count)
    full = (count > 0) & (count >= min_points)
    height = np.full(cells, np.nan, np.float32)
    height[full] = unkey(ks[start[full] + t[full]])
    return height.reshape(grid.shape), count.astype(np.int32).reshape(grid.shape)


def fill_numpy(h, radius):
    """One MovingAverage pass: empty (NaN) cells get the fp64 mean (dy outer, dx inner) of the window's non-empty cells."""
    h = np.asarray(h, np.float32)
    H, W = h.shape
    r = int(radius)
    pad = np.full((H + 2 * r, W + 2 * r), np.nan, np.float32)
    pad[r:r + H, r:r + W] = h
    s, n = np.zeros((H, W)), np.zeros((H, W), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            a = pad[r + dy:r + dy + H, r + dx:r + dx + W]
            m = ~np.isnan(a)
            s += np.where(m, a.astype(np.float64), 0.0)
            n += m
    out = h.copy()
    e = np.isnan(h) & (n > 0)
    out[e] = (s[e] / n[e]).astype(np.float32)
    return out


# ----------------------------------------------------------------------------------------
def test_numpy_restatement_on_a_hand_example():
    g = dsm.DsmGrid([0.0, 3.0, 0.0, 2.0], [1.0, 1.0])
    pts = np.array([[0.5, 1.5, 5.0], [0.2, 1.9, 7.0], [0.9, 1.1, -0.0], [2.5, 0.5, 0.0], [2.5, 0.5, -0.0], [3.0, 0.5, 9.0],
                    [1.5, 0.0, 4.0], [1.5, 2.5, 4.0], [np.nan, 1.0, 1.0]], np.float32)
    h, c = dsm_numpy(pts, g)
    assert c.tolist() == [[3, 0, 0], [0, 0, 2]]      # (3.0, .) is on Xmax, (., 0.0) on Ymin: outside; y 2.5 north of Ymax
    assert h[0, 0] == 7.0 and np.isnan(h[0, 1]) and h[1, 2] == 0.0 and not np.signbit(h[1, 2])   # +0.0 > -0.0
    h2, _ = dsm_numpy(pts, g, "Robust_Max", trim=0.5)
    assert h2[0, 0] == 5.0 and np.signbit(h2[1, 2])  # t = floor(0.5 * n): 1 of 3, 1 of 2 dropped
    h3, _ = dsm_numpy(pts, g, min_points=3)
    assert h3[0, 0] == 7.0 and np.isnan(h3[1, 2])
    f = fill_numpy(h, 1)
    assert f[0, 1] == np.float32((7.0 + 0.0) / 2) and f[0, 0] == 7.0 and np.isnan(fill_numpy(np.full((2, 2), np.nan), 1)).all()


def test_grid_size_and_world_file_follow_the_reference():
    border, unit = [-430.0, 150.0, -330.0, 250.0, 700.0, 900.0], [0.2, 0.2]   # the reference's config.yaml CREATEDSM
    g = dsm.DsmGrid(border, unit)
    assert (g.width, g.height) == (int((150.0 + 430.0 + 0.00000001) / 0.2), int((250.0 + 330.0 + 0.00000001) / 0.2)) == (2900, 2900)
    assert (g.z_min, g.z_max) == (700.0, 900.0)
    assert g.tfw_text() == "0.2\n0\n0\n-0.2\n-430.0\n250.0"
    g2 = dsm.DsmGrid([0, 10.5, -3, 7], (0.3, 0.7))
    assert (g2.width, g2.height) == (int((10.5 + 0.00000001) / 0.3), int((10 + 0.00000001) / 0.7))
    assert g2.tfw_text() == str(0.3) + "\n0\n0\n" + str(-0.7) + "\n" + str(0.0) + "\n" + str(7.0)
    assert (g2.z_min, g2.z_max) == (-math.inf, math.inf)
    g3 = dsm.DsmGrid(border, unit, size=(2000, 1500))   # an explicit dsm_size wins
    assert g3.shape == (1500, 2000) and g3.tfw_text() == g.tfw_text()
    for bad in (dict(border=border, unit=[0.0, 0.2]), dict(border=border, unit=[0.2, -1]), dict(border=border[:3], unit=unit),
                dict(border=border, unit=unit, size=(0, 10)), dict(border=border, unit=unit, size=(1 << 16, 1 << 15))):
        with pytest.raises(ValueError):
            dsm.DsmGrid(**bad)


def test_tiff_round_trips_through_pil(tmp_path):
    from PIL import Image

    g = dsm.DsmGrid([-10.0, 27.0, 5.0, 1005.0], [1.0, 1.0])   # 37 x 1000: several strips
    rng = np.random.default_rng(0)
    h = (rng.standard_normal(g.shape) * 100).astype(np.float32)
    h[3, 4] = np.nan
    h[10:20, :] = np.nan
    h[0, 0], h[0, 1] = -0.0, np.float32(1e-42)
    tif, tfw = dsm.write_dsm(str(tmp_path / "d.tif"), torch.from_numpy(h), g, nodata=-9999.0)
    assert tfw == str(tmp_path / "d.tfw") and open(tfw).read() == g.tfw_text()
    im = Image.open(tif)
    assert im.mode == "F" and im.size == (g.width, g.height)
    got = np.array(im)
    want = np.where(np.isnan(h), np.float32(-9999.0), h)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    tags = im.tag_v2
    assert tuple(np.ravel(tags[339])) == (3,) and tuple(np.ravel(tags[258])) == (32,)
    assert tuple(tags[33550]) == (1.0, 1.0, 0.0)
    assert tuple(tags[33922]) == (0.0, 0.0, 0.0, -10.0, 1005.0, 0.0)
    assert tuple(tags[34735]) == (1, 1, 0, 1, 1025, 0, 1, 1)   # PixelIsArea, no CRS key
    assert tags[42113] == "-9999"
    dsm.write_dsm(str(tmp_path / "e.tif"), h, g, nodata=0.5)
    assert Image.open(str(tmp_path / "e.tif")).tag_v2[42113] == "0.5"
    assert np.array(Image.open(str(tmp_path / "e.tif")))[3, 4] == np.float32(0.5)
    with pytest.raises(ValueError, match="does not match"):
        dsm.write_dsm(str(tmp_path / "f.tif"), h[1:], g)


def test_rasters_over_4_gib_are_refused_before_allocating(tmp_path):
    g = dsm.DsmGrid([0.0, 1.0, 0.0, 1.0], [1.0, 1.0], size=(40000, 30000))   # 4.47 GiB of float32
    with pytest.raises(ValueError, match="4 GiB"):
        dsm.write_dsm(str(tmp_path / "big.tif"), np.zeros((1, 1), np.float32), g)
    assert not (tmp_path / "big.tif").exists() and not (tmp_path / "big.tfw").exists()


def test_header_binding_and_library_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_version() == 11
    assert lib.d3d_dsm_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_dsm_scratch_bytes(1000, 30, 20, 0) >= 30 * 20 * 4
    assert lib.d3d_dsm_scratch_bytes(1000, 30, 20, 1) >= 2 * 1000 * 4 + 30 * 20 * 4
    assert lib.d3d_dsm_scratch_bytes(-1, 30, 20, 1) == 0 and lib.d3d_dsm_scratch_bytes(10, 0, 20, 1) == 0
    assert lib.d3d_dsm_scratch_bytes(10, 30, 20, 2) == 0


def test_invalid_arguments_are_reported_before_any_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below fails its checks first
    h, c = ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    big = 1 << 40
    ok = dict(xyz=fake, n=10, xmin=0.0, ymax=10.0, ux=1.0, uy=1.0, zmin=-math.inf, zmax=math.inf, W=10, H=10, select=1, trim=0.1,
              minp=1, scratch=fake, sbytes=big, height=h, count=c)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.d3d_dsm_from_points(a["xyz"], a["n"], a["xmin"], a["ymax"], a["ux"], a["uy"], a["zmin"], a["zmax"], a["W"], a["H"],
                                       a["select"], a["trim"], a["minp"], a["scratch"], a["sbytes"], a["height"], a["count"], None)

    cases = [(dict(ux=0.0), b"unit"), (dict(uy=-0.2), b"unit"), (dict(ux=math.nan), b"unit"), (dict(ux=math.inf), b"unit"),
             (dict(W=0), b"raster"), (dict(H=0), b"raster"), (dict(W=1 << 16, H=1 << 15), b"raster"), (dict(W=-3), b"raster"),
             (dict(trim=1.0), b"trim"), (dict(trim=-0.01), b"trim"), (dict(trim=math.nan), b"trim"),
             (dict(xyz=None), b"null"), (dict(height=None), b"null"), (dict(count=None), b"null"), (dict(scratch=None), b"null"),
             (dict(sbytes=16), b"scratch"), (dict(n=-1), b"n_points"), (dict(n=1 << 31), b"n_points"), (dict(select=2), b"select"),
             (dict(minp=0), b"min_points"), (dict(zmin=5.0, zmax=4.0), b"z bounds"), (dict(xmin=math.inf), b"border")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.d3d_last_error(), (kw, lib.d3d_last_error())
    for r in (0, 17, -1):
        assert lib.d3d_dsm_fill_moving_average(fake, h, 10, 10, r, None) == -1
        assert b"radius" in lib.d3d_last_error()
    assert lib.d3d_dsm_fill_moving_average(None, h, 10, 10, 2, None) == -1 and b"null" in lib.d3d_last_error()
    assert lib.d3d_dsm_fill_moving_average(fake, None, 10, 10, 2, None) == -1 and b"null" in lib.d3d_last_error()
    assert lib.d3d_dsm_fill_moving_average(fake, fake, 10, 10, 2, None) == -1 and b"alias" in lib.d3d_last_error()
    assert lib.d3d_dsm_fill_moving_average(fake, h, 0, 10, 2, None) == -1 and b"raster" in lib.d3d_last_error()


def test_operator_refuses_cpu_tensors_and_bad_settings():
    g = dsm.DsmGrid([0, 10, 0, 10], [1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsm.points_to_dsm(torch.zeros(5, 3), g)
    with pytest.raises(ValueError, match="select"):
        dsm.points_to_dsm(torch.zeros(5, 3), g, select="Median")
    with pytest.raises(ValueError, match="interpolation"):
        dsm.points_to_dsm(torch.zeros(5, 3), g, interpolation="Kriging")
    with pytest.raises(ValueError, match="radius"):
        dsm.points_to_dsm(torch.zeros(5, 3), g, interpolation="MovingAverage", radius=17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsm.fill_moving_average(torch.zeros(4, 4))


def test_predict_dsm_flags_are_off_by_default_and_need_fuse():
    a = predict.parse_args(["--output_folder", "o"])
    assert a.dsm is None and a.dsm_border is None and a.dsm_size is None and a.dsm_select == "Max"
    assert a.dsm_interpolation == "none" and a.dsm_trim == 0.1 and a.dsm_min_points == 1 and a.dsm_nodata == -9999.0
    b = predict.parse_args(["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=-1,2,-3,4,5,6", "--dsm_unit=0.5",
                            "--dsm_size=7,8", "--dsm_select", "Robust_Max", "--dsm_trim", "0.2", "--dsm_min_points", "3",
                            "--dsm_interpolation", "MovingAverage", "--dsm_radius", "4", "--dsm_iterations", "2", "--dsm_nodata", "0"])
    s = predict._dsm_settings(b)
    assert s == {"path": "x.tif", "border": [-1.0, 2.0, -3.0, 4.0, 5.0, 6.0], "unit": [0.5, 0.5], "size": [7, 8],
                 "select": "Robust_Max", "trim": 0.2, "min_points": 3, "interpolation": "MovingAverage", "radius": 4,
                 "iterations": 2, "nodata": 0.0}
    with pytest.raises(SystemExit):
        predict.parse_args(["--output_folder", "o", "--dsm", "x.tif", "--dsm_border=0,1,0,1"])   # no --fuse
    with pytest.raises(SystemExit):
        predict.parse_args(["--output_folder", "o", "--fuse", "--dsm", "x.tif"])                  # no border
    with pytest.raises(SystemExit):
        predict.parse_args(["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0"])


CREATEDSM = {"run_create_dsm": True, "dsm_source": "pc", "pc_select_method": "Robust_Max", "pc_interpolation_method": None,
             "dsm_uint": [0.2, 0.2], "dsm_size": [2900, 2900], "bbx_border_dsm": [-430.0, 150.0, -330.0, 250.0, 700.0, 900.0]}


def test_mvs_dl_reads_createdsm_and_formats_the_flags_only_when_asked():
    s = mvs_dl.dsm_settings({"CREATEDSM": CREATEDSM})
    assert s["select"] == "Robust_Max" and s["interpolation"] is None and s["unit"] == [0.2, 0.2] and s["size"] == [2900, 2900]
    assert s["border"] == CREATEDSM["bbx_border_dsm"] and s["run_create_dsm"] is True
    assert mvs_dl.dsm_settings(dict(CREATEDSM, pc_interpolation_method="MovingAverage"))["interpolation"] == "MovingAverage"
    assert mvs_dl.dsm_settings(dict(CREATEDSM, pc_interpolation_method="none"))["interpolation"] is None
    with pytest.raises(Exception, match="Not implemented yet!"):
        mvs_dl.dsm_settings({"CREATEDSM": dict(CREATEDSM, dsm_source="mesh")})
    kw = dict(pretrain_weight="w.ckpt")
    plain = mvs_dl.MVS_Inference(64, 32, **kw).argv("d", "m")
    assert not any(x.startswith("--dsm") for x in plain)
    asked = mvs_dl.MVS_Inference(64, 32, dsm=dict(s, path="out/dsm.tif"), extra_args=["--fuse"], **kw).argv("d", "m")
    extra = [x for x in asked if x not in plain]
    assert extra == ["--dsm=out/dsm.tif", "--dsm_border=-430.0,150.0,-330.0,250.0,700.0,900.0", "--dsm_unit=0.2,0.2",
                     "--dsm_size=2900,2900", "--dsm_select=Robust_Max", "--fuse"]
    a = predict.parse_args(["--output_folder", "o"] + extra)
    assert predict._dsm_settings(a) == dict({k: v for k, v in s.items() if k != "run_create_dsm"}, path="out/dsm.tif")
    with pytest.raises(ValueError, match="path"):
        mvs_dl.MVS_Inference(64, 32, dsm=s, **kw).argv("d", "m")
