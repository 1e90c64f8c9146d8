"""The terrain filter (deep3d_aerial_amd/dtm.py) without a GPU: the level table by hand, the properties of the
numpy restatement (tests/dtm_scene.py) and what it does on the analytic scene, and the argument errors and flags of the Python
layer.  The kernels are held to the restatement bit for bit in tests/test_dtm_gpu.py."""
import numpy as np
import pytest
import torch

import dtm_scene as S
from deep3d_aerial_amd import _lib, dtm, predict
from deep3d_aerial_amd.dsm import DsmGrid

F = lambda v: float(np.float32(v))


def _grid(ux, uy, W=8, H=8):
    return DsmGrid([0.0, W * ux, 0.0, H * uy], [ux, uy], size=(W, H))


# ----------------------------------------------------------------------------------------
# the level table
# ----------------------------------------------------------------------------------------
def test_levels_square_units_by_hand():
    # u = 1: a = 1, 2, 4; 2 a + u = 3, 5, 9 -> the stop rule holds with equality at k = 3 for max_window 9
    # dh = min(2.5, 0.3 + 0.6 (a_k - a_(k-1))) = 0.9, 0.9, 1.5
    assert dtm.levels(_grid(1.0, 1.0), 9.0, 0.3, 0.3, 2.5) == [(1, 1, F(0.3 + 0.6 * 1.0)), (2, 2, F(0.3 + 0.6 * 1.0)), (4, 4, F(0.3 + 0.6 * 2.0))]
    # one cell more and a fourth level is needed: a = 8, dh = min(2.5, 0.3 + 0.6 * 4) = 2.5
    got = dtm.levels(_grid(1.0, 1.0), 9.0 + 1e-9, 0.3, 0.3, 2.5)
    assert len(got) == 4 and got[3] == (8, 8, F(2.5))
    # a window no wider than 3 cells is one level
    assert dtm.levels(_grid(1.0, 1.0), 3.0, 0.0, 0.25, 0.25) == [(1, 1, 0.25)]
    # the defaults on a 0.1 grid: 2 a + 0.1 >= 40 first at a = 25.6 (k = 9), radius 256
    d = dtm.levels(_grid(0.1, 0.1))
    assert [r for r, _, _ in d] == [1, 2, 4, 8, 16, 32, 64, 128, 256] and d[0][2] == F(0.3 + 0.6 * 0.1) and d[-1][2] == F(2.5)
    assert dtm.DEFAULTS == S.DEFAULTS == {"max_window": 40.0, "slope": 0.3, "dh0": 0.3, "dh_max": 2.5}


def test_levels_non_square_units_by_hand():
    # ux = 0.5, uy = 0.2: u = 0.5, a = 0.5, 1, 2; rx = a / 0.5 = 1, 2, 4; ry = floor(a / 0.2 + 0.5) = floor(3.0) = 3 (2.5 + 0.5),
    # 5, 10; 2 a + u = 1.5, 2.5, 4.5 >= 4.5 at k = 3; dh = 0.1 + 2 * 0.5 * (0.5, 0.5, 1.0) = 0.6, 0.6, 1.1 -> capped at 1.0
    got = dtm.levels(_grid(0.5, 0.2), 4.5, 0.5, 0.1, 1.0)
    assert got == [(1, 3, F(0.6)), (2, 5, F(0.6)), (4, 10, F(1.0))]
    # the coarser axis never gets a radius below 1, whatever the ratio
    assert dtm.levels(_grid(0.1, 1.0), 3.0)[0][:2] == (10, 1)
    for unit in ((1.0, 1.0), (0.5, 0.2), (0.25, 0.5)):
        for mw in (3.0, 9.0, 16.5, 40.0):
            want = S.levels(unit, mw, 0.3, 0.3, 2.5)
            got = dtm.levels(_grid(*unit), mw)
            assert [(a, b, np.float32(c)) for a, b, c in got] == want


def test_levels_refuse_a_radius_above_the_cap():
    assert dtm.MAX_RADIUS == _lib.CONSTANTS["D3D_DTM_MAX_RADIUS"] == S.MAX_RADIUS == 1024
    # u = 1: radius 1024 is level 11 (2 a + u = 2049); 2050 needs radius 2048
    assert dtm.levels(_grid(1.0, 1.0), 2049.0)[-1][:2] == (1024, 1024)
    with pytest.raises(ValueError, match="above 1024"):
        dtm.levels(_grid(1.0, 1.0), 2050.0)
    # non-square: ux = 0.001, uy = 1: the first level has rx = 1000, the second would need 2000
    assert dtm.levels(_grid(0.001, 1.0), 3.0) == [(1000, 1, F(0.9))]
    with pytest.raises(ValueError, match="above 1024"):
        dtm.levels(_grid(0.001, 1.0), 3.5)


@pytest.mark.parametrize("bad", [dict(max_window=0.0), dict(max_window=-1.0), dict(max_window=float("inf")), dict(slope=-0.1),
                                 dict(slope=float("nan")), dict(dh0=-0.1), dict(dh0=3.0), dict(dh_max=float("inf")),
                                 dict(dh_max="2"), dict(max_window=True)])
def test_parameters_are_checked(bad):
    with pytest.raises(ValueError):
        dtm.levels(_grid(1.0, 1.0), **bad)
    with pytest.raises(ValueError):
        dtm.check_settings(dict({"path": "t.tif"}, **bad))


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def _noise(shape, seed, nan_share=0.0):
    rng = np.random.default_rng(seed)
    h = (rng.integers(-16, 17, shape) / 4.0).astype(np.float32)
    h[rng.random(shape) < nan_share] = np.nan
    return h


def test_restatement_walks_the_window():
    h = _noise((9, 11), 0, 0.2)
    h[2:6, 3:8] = np.nan                       # an island larger than the window
    h[0, 0], h[0, 1] = -0.0, 0.0
    for rx, ry in ((1, 1), (2, 1), (1, 3), (20, 20)):
        for smallest in (True, False):
            assert S.same_bits(S._extreme(h, rx, ry, smallest), S.brute(h, rx, ry, smallest))
    assert np.signbit(S.erode(h, 1, 1)[0, 0]) and not np.signbit(S.dilate(h, 1, 1)[0, 0])   # -0.0 < +0.0
    assert np.isnan(S.erode(h, 1, 1)[3, 5]) and np.isnan(S.dilate(h, 1, 1)[4, 5])            # the window holds no value
    assert S.bits(S.erode(h, 1, 1))[3, 5] == 0x7fc00000
    full = _noise((12, 17), 1)
    ref = S.scipy_cross_check(full, 2, 3)
    if ref is not None:
        assert np.array_equal(ref[0], S.erode(full, 2, 3)) and np.array_equal(ref[1], S.dilate(full, 2, 3))


def test_opening_is_anti_extensive_and_idempotent():
    h = _noise((40, 37), 2, 0.15)
    for rx, ry in ((1, 1), (3, 2), (8, 8)):
        o = S.open_(h, rx, ry)
        ok = ~np.isnan(h)
        assert not np.isnan(o[ok]).any() and (S.key(o[ok]) <= S.key(h[ok])).all()
    full = _noise((40, 37), 3)
    for rx, ry in ((1, 1), (3, 2), (8, 8)):
        o = S.open_(full, rx, ry)
        assert S.same_bits(S.open_(o, rx, ry), o)


def test_pull_push_keeps_values_and_fills_from_one_cell():
    h = _noise((13, 9), 4, 0.6)
    filled = S.fill_pull_push(h)
    ok = ~np.isnan(h)
    assert not np.isnan(filled).any() and np.array_equal(S.bits(filled)[ok], S.bits(h)[ok])
    assert filled.min() >= h[ok].min() and filled.max() <= h[ok].max()       # means of means
    for shape, at in (((1, 1), (0, 0)), ((1, 7), (0, 6)), ((5, 3), (4, 0)), ((33, 20), (0, 0))):
        one = np.full(shape, np.nan, np.float32)
        one[at] = 2.5
        assert np.array_equal(S.fill_pull_push(one), np.full(shape, 2.5, np.float32))
    none = S.fill_pull_push(np.full((5, 6), np.nan, np.float32))
    assert (S.bits(none) == 0x7fc00000).all()
    # a parent is the fp64 mean of its children rounded once; a pushed cell weighs its parents 9 : 3 : 3 : 1
    assert S.pull(np.array([[1.0, np.nan], [2.0, 4.0]], np.float32))[0, 0] == np.float32(7.0 / 3.0)
    coarse = np.array([[1.0, 2.0], [3.0, 5.0]], np.float32)
    got = S.push(coarse, np.full((4, 4), np.nan, np.float32))
    assert got[1, 1] == np.float32((9 * 1.0 + 3 * 2.0 + 3 * 3.0 + 5.0) / 16.0) and got[0, 0] == 1.0
    assert got[0, 1] == np.float32((9 * 1.0 + 3 * 2.0) / 12.0) and got[3, 2] == np.float32((9 * 5.0 + 3 * 3.0) / 12.0)


@pytest.fixture(scope="module")
def large():
    sc = S.scene(S.LARGE)
    return sc, S.dsm_to_dtm(sc["height"], sc["unit"], max_window=sc["max_window"], **{k: S.DEFAULTS[k] for k in ("slope", "dh0", "dh_max")})


def _interior(mask):
    m = mask.copy()
    m[1:] &= mask[:-1]
    m[:-1] &= mask[1:]
    m[:, 1:] &= mask[:, :-1]
    m[:, :-1] &= mask[:, 1:]
    return m


def test_scene_buildings_are_struck_and_the_wide_one_is_kept(large):
    sc, (dtm_, level, ndsm) = large
    ux, uy = sc["unit"]
    widths = []
    for b in range(1, sc["wide"] + 1):
        m = sc["building"] == b
        rows, cols = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
        narrow = min(len(rows) * uy, len(cols) * ux)
        widths.append(narrow)
        roof = _interior(m) if _interior(m).any() else m
        if b == sc["wide"]:
            assert narrow > sc["max_window"] and (level[roof] == 0).all()      # the stated limit of the method
            continue
        assert narrow < sc["max_window"] and (level[roof] > 0).all(), b
        # the terrain under it, filled from the ground around, stays within dh_max of the truth
        assert np.abs(dtm_[m] - sc["terrain"][m]).max() < S.DEFAULTS["dh_max"], b
        assert (ndsm[roof] > 3.0).all()
    assert max(widths[:-1]) >= sc["max_window"] - 1.0                            # one building just under max_window
    small = sc["object"] & (sc["building"] == 0)
    assert small.sum() >= 40 and (level[small] > 0).all()                        # trees and spikes


def test_scene_bare_terrain_is_kept(large):
    sc, (dtm_, level, ndsm) = large
    bare = ~sc["object"] & ~sc["hole"]
    assert bare.sum() > 20000 and (level[bare] == 0).mean() >= 0.99
    assert (level[sc["hole"]] == 255).all() and sc["hole"].sum() > 150 and not (level[~sc["hole"]] == 255).any()
    assert not np.isnan(dtm_).any() and np.isnan(ndsm[sc["hole"]]).all() and not np.isnan(ndsm[~sc["hole"]]).any()
    assert np.array_equal(S.bits(dtm_)[level == 0], S.bits(sc["height"])[level == 0])
    # the terrain's gradient stays well under the slope the thresholds allow for
    gy, gx = np.gradient(sc["terrain"], sc["unit"][1], sc["unit"][0])
    assert np.hypot(gx, gy).max() < 0.15
    assert (np.round(sc["height"][~sc["hole"]].astype(np.float64) * 64) == sc["height"][~sc["hole"]].astype(np.float64) * 64).all()


# ----------------------------------------------------------------------------------------
# the Python layer without a GPU
# ----------------------------------------------------------------------------------------
def test_the_library_exports_the_terrain_entry_points():
    names = ("d3d_dtm_scratch_bytes", "d3d_dtm_erode", "d3d_dtm_dilate", "d3d_dtm_open", "d3d_dtm_classify", "d3d_dtm_ground",
             "d3d_dtm_ndsm", "d3d_dtm_pull", "d3d_dtm_push")
    assert all(n in _lib.SIGNATURES for n in names)
    lib = _lib.load()
    assert lib.d3d_dtm_scratch_bytes(100, 50) >= 2 * 100 * 50 * 4
    assert lib.d3d_dtm_scratch_bytes(0, 5) == 0 and lib.d3d_dtm_scratch_bytes(1 << 16, 1 << 15) == 0


def test_argument_errors_need_no_gpu():
    g = _grid(1.0, 1.0, 6, 4)
    ok = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtm.erode(ok, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtm.dsm_to_dtm(ok, g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtm.fill_pull_push(ok)
    for bad in (torch.zeros(4, 6, dtype=torch.float64), torch.zeros(6), torch.zeros(2, 4, 6), torch.zeros(0, 6),
                torch.zeros(4, 6, dtype=torch.int32)):
        for call in (lambda t: dtm.erode(t, 1, 1), lambda t: dtm.dilate(t, 1, 1), lambda t: dtm.open_(t, 1, 1), dtm.fill_pull_push):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match="does not match the grid"):
        dtm.classify_ground(torch.zeros(6, 4), g)
    for r in ((0, 1), (1, 0), (1025, 1), (1, 1025), (1.5, 1), (True, 1)):
        with pytest.raises(ValueError, match="radius"):
            dtm.open_(ok, *r)
    with pytest.raises(ValueError, match="max_window"):
        dtm.dsm_to_dtm(ok, g, max_window=0.0)
    with pytest.raises(ValueError, match="above 1024"):
        dtm.dsm_to_dtm(ok, g, max_window=5000.0)
    with pytest.raises(TypeError):
        dtm.dsm_to_dtm(ok, "grid")
    with pytest.raises(TypeError):
        dtm.erode(np.zeros((4, 6), np.float32), 1, 1)
    for s in ({}, {"path": "t.tiff"}, {"path": "t.tif", "ndsm": "n.png"}, {"path": "t.tif", "ground": 3}, {"path": "t.tif", "dh0": 9.0}):
        with pytest.raises(ValueError):
            dtm.check_settings(s)
    assert dtm.check_settings({"path": "t.tif", "ndsm": "n.tif", "slope": 0.1}) == (40.0, 0.1, 0.3, 2.5)


def test_cli_flags():
    a = dtm.parser().parse_args(["--dsm", "d.tif", "--out", "t.tif"])
    assert dtm.settings_from_args(a, a.out) == {"path": "t.tif", "ndsm": None, "ground": None, "max_window": 40.0, "slope": 0.3,
                                                "dh0": 0.3, "dh_max": 2.5, "nodata": -9999.0}
    b = dtm.parser().parse_args(["--dsm", "d.tif", "--out", "t.tif", "--ndsm", "n.tif", "--ground", "g.tif", "--max_window", "12.5",
                                 "--slope", "0.2", "--dh0", "0.1", "--dh_max", "1.5", "--nodata", "0"])
    assert dtm.settings_from_args(b, b.out) == {"path": "t.tif", "ndsm": "n.tif", "ground": "g.tif", "max_window": 12.5, "slope": 0.2,
                                                "dh0": 0.1, "dh_max": 1.5, "nodata": 0.0}
    for argv in (["--out", "t.tif"], ["--dsm", "d.tif"], ["--dsm", "d.tif", "--out", "t.png"],
                 ["--dsm", "d.tif", "--out", "t.tif", "--dh0", "3"], ["--dsm", "d.tif", "--out", "t.tif", "--max_window", "0"]):
        with pytest.raises(SystemExit):
            dtm.main(argv)


def test_predict_dtm_flags_are_off_by_default_and_need_dsm():
    a = predict.parse_args(["--output_folder", "o"])
    assert a.dtm is None and a.dtm_ndsm is None and a.dtm_ground is None
    assert (a.dtm_max_window, a.dtm_slope, a.dtm_dh0, a.dtm_dh_max) == (40.0, 0.3, 0.3, 2.5)
    for source in (["--dsm_source", "pc"], ["--dsm_source", "mesh", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1", "--mesh_voxel", "0.1"]):
        b = predict.parse_args(["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0,1", "--dsm_nodata", "-1",
                                "--dtm", "t.tif", "--dtm_ndsm", "n.tif", "--dtm_ground", "g.tif", "--dtm_max_window", "20",
                                "--dtm_slope", "0.2", "--dtm_dh0", "0.1", "--dtm_dh_max", "2"] + source)
        assert predict._dtm_settings(b) == {"path": "t.tif", "ndsm": "n.tif", "ground": "g.tif", "max_window": 20.0, "slope": 0.2,
                                            "dh0": 0.1, "dh_max": 2.0, "nodata": -1.0}
    with pytest.raises(SystemExit):
        predict.parse_args(["--output_folder", "o", "--fuse", "--dtm", "t.tif"])                                  # no --dsm
    with pytest.raises(SystemExit):
        predict.parse_args(["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0,1", "--dtm", "t.tif", "--dtm_dh0", "9"])


def test_predict_and_fuse_refuses_dtm_without_dsm():
    from deep3d_aerial_amd import pipeline

    with pytest.raises(ValueError, match="dtm needs dsm"):
        pipeline.predict_and_fuse(None, [], "o", dtm={"path": "t.tif"})
    with pytest.raises(ValueError, match="max_window"):
        pipeline.predict_and_fuse(None, [], "o", dsm={"path": "d.tif", "border": [0, 1, 0, 1]}, dtm={"path": "t.tif", "max_window": -1.0})
