"""The object segmentation (deep3d_aerial_amd/objects.py) without a GPU: min_cells by hand, the properties of the
numpy restatement (tests/objects_scene.py) and what it finds on the analytic scene, and the argument errors, flags and CSV bytes of
the Python layer.  The kernels are held to the restatement bit for bit in tests/test_objects_gpu.py."""
import numpy as np
import pytest
import torch

import objects_scene as S
from deep3d_aerial_amd import _lib, objects, predict
from deep3d_aerial_amd.dsm import DsmGrid


def _grid(ux, uy, W=8, H=8):
    return DsmGrid([0.0, W * ux, 0.0, H * uy], [ux, uy], size=(W, H))


# ----------------------------------------------------------------------------------------
# min_cells, radii, parameters
# ----------------------------------------------------------------------------------------
def test_min_cells_by_hand():
    # square units: 0.5 x 0.5 = 0.25 per cell; 10 / 0.25 = 40 exactly (equality: 40 cells are enough), a hair more needs 41
    assert objects.min_cells(_grid(0.5, 0.5), 10.0) == 40 == S.min_cells((0.5, 0.5), 10.0)
    assert objects.min_cells(_grid(0.5, 0.5), 10.0 + 1e-9) == 41
    assert objects.min_cells(_grid(0.5, 0.5), 9.9) == 40 and objects.min_cells(_grid(0.5, 0.5), 9.75) == 39
    # non-square: 0.5 x 0.25 = 0.125 per cell; 10 / 0.125 = 80; 1 / 0.125 = 8; 1.01 / 0.125 = 8.08 -> 9
    assert objects.min_cells(_grid(0.5, 0.25), 10.0) == 80 == S.min_cells((0.5, 0.25), 10.0)
    assert objects.min_cells(_grid(0.5, 0.25), 1.0) == 8 and objects.min_cells(_grid(0.5, 0.25), 1.01) == 9
    # never below one cell
    assert objects.min_cells(_grid(1.0, 1.0), 0.0) == 1 and objects.min_cells(_grid(2.0, 3.0), 5.0) == 1
    assert objects.min_cells(_grid(1.0, 1.0), 1.0) == 1 and objects.min_cells(_grid(1.0, 1.0), 1.5) == 2
    assert objects.min_cells(_grid(0.1, 0.1)) == 1000
    assert objects.DEFAULTS == S.DEFAULTS == {"min_height": 2.0, "min_area": 10.0, "connectivity": 8, "open": 0.0}
    assert objects.COLUMNS == S.COLUMNS


def test_open_radii_by_hand():
    assert objects.open_radii(_grid(0.5, 0.5), 0.0) is None
    # floor(open / u + 0.5): 1.0 / 0.5 = 2; 0.6 / 0.5 = 1.2 -> 1; 0.75 / 0.5 = 1.5 -> 2; non-square (0.5, 0.25): 1 and 2
    assert objects.open_radii(_grid(0.5, 0.5), 1.0) == (2, 2) and objects.open_radii(_grid(0.5, 0.5), 0.6) == (1, 1)
    assert objects.open_radii(_grid(0.5, 0.5), 0.75) == (2, 2) and objects.open_radii(_grid(0.5, 0.25), 0.5) == (1, 2)
    assert objects.MAX_RADIUS == 1024 and objects.open_radii(_grid(1.0, 1.0), 1024.0) == (1024, 1024)
    for g, o in ((_grid(1.0, 1.0), 0.4), (_grid(1.0, 1.0), 1025.0), (_grid(0.5, 4.0), 1.0)):   # a radius of 0, above the cap, 0 on one axis
        with pytest.raises(ValueError, match="outside 1..1024"):
            objects.open_radii(g, o)
        with pytest.raises(ValueError):
            S.foreground(np.zeros((4, 4), np.float32), g.unit, 2.0, o)


@pytest.mark.parametrize("bad", [dict(min_height=-0.1), dict(min_height=float("nan")), dict(min_height="2"), dict(min_area=-1.0),
                                 dict(min_area=float("inf")), dict(connectivity=6), dict(connectivity=8.0), dict(connectivity=True),
                                 dict(open=-1.0), dict(open=float("inf")), dict(min_height=True)])
def test_parameters_are_checked(bad):
    with pytest.raises(ValueError):
        objects.check_params(**bad)
    with pytest.raises(ValueError):
        objects.check_settings(dict({"path": "o.tif"}, **bad))


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def test_restatement_roots_by_hand_and_against_scipy():
    m = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 1],
                  [0, 0, 0, 0],
                  [1, 1, 0, 1]], bool)
    assert S.roots(m, 4).tolist() == [[0, -1, -1, 3], [-1, 5, -1, 3], [-1, -1, -1, -1], [12, 12, -1, 15]]
    assert S.roots(m, 8).tolist() == [[0, -1, -1, 3], [-1, 0, -1, 3], [-1, -1, -1, -1], [12, 12, -1, 15]]
    for name, p in S.patterns(37, 29).items():
        for conn in (4, 8):
            r = S.roots(p, conn)
            assert ((r >= 0) == p).all() and (r[p] <= np.arange(p.size).reshape(p.shape)[p]).all(), name
            assert (r.ravel()[r[p]] == r[p]).all(), name                         # a root is its own root
            ref = S.scipy_cross_check(p, conn)
            if ref is not None:
                assert np.array_equal(ref, r), (name, conn)
    # what the patterns are for
    assert len(np.unique(S.roots(S.checkerboard(6, 7), 4))) == 21 + 1 and set(np.unique(S.roots(S.checkerboard(6, 7), 8))) == {-1, 0}
    for name in ("serpentine", "u", "comb", "diagonal"):
        p = S.patterns(37, 29)[name]
        assert set(np.unique(S.roots(p, 8))) == {-1, 0}, name
    assert len(np.unique(S.roots(S.diagonal(9, 9), 4))) == 9 + 1                  # every cell of the diagonal alone (and -1)
    plain, joined = S.rings(21, 21), S.rings(21, 21, True)
    assert len(np.unique(S.roots(plain, 8))) == 1 + 6 and len(np.unique(S.roots(joined, 8))) < 1 + 6
    assert len(np.unique(S.roots(joined, 4))) > len(np.unique(S.roots(joined, 8)))


def test_restatement_statistics_and_table_by_hand():
    h = np.full((4, 5), np.nan, np.float32)
    h[0, 0:3] = [2.0, 3.5, 2.25]            # one object of three cells
    h[2, 4], h[3, 4] = 9.0, 1.0             # one cell (the 1.0 is below min_height)
    h[3, 0] = np.inf                        # not finite: background
    label, t = S.segment(h, (0.5, 2.0), (10.0, 100.0), min_height=2.0, min_area=0.0, connectivity=4)
    assert label.tolist() == [[1, 1, 1, 0, 0], [0] * 5, [0, 0, 0, 0, 2], [0] * 5]
    assert t["id"].tolist() == [1, 2] and t["cells"].tolist() == [3, 1] and t["area"].tolist() == [3.0, 1.0]
    assert t["x"].tolist() == [10.0 + (1.0 + 0.5) * 0.5, 10.0 + 4.5 * 0.5] and t["y"].tolist() == [100.0 - 0.5 * 2.0, 100.0 - 2.5 * 2.0]
    assert [t[k].tolist() for k in ("i0", "i1", "j0", "j1")] == [[0, 2], [0, 2], [0, 4], [2, 4]]
    assert t["height_max"].tolist() == [3.5, 9.0] and t["height_mean"].tolist() == [7.75 / 3.0, 9.0] and t["volume"].tolist() == [7.75, 9.0]
    # q rounds half up at 1/1024 and saturates
    assert S.q(np.float32([0.0, 1.0 / 2048, 1.0 / 4096, 3.0, 3.4e38])).tolist() == [0, 1, 0, 3072, 2 ** 32 - 1]
    # min_area 1.5 on cells of 1.0: two cells needed, the single cell is dropped and the ids stay dense
    label, t = S.segment(h, (0.5, 2.0), (10.0, 100.0), min_height=2.0, min_area=1.5, connectivity=4)
    assert label.max() == 1 and t["id"].tolist() == [1] and label[2, 4] == 0


@pytest.fixture(scope="module")
def large():
    return S.scene(S.LARGE)


def test_scene_buildings_are_objects(large):
    sc = large
    params = dict(min_height=2.0, min_area=10.0, open=0.0)               # the defaults: 40 cells of 0.5 x 0.5
    need = S.min_cells(sc["unit"], params["min_area"])
    assert need == 40
    label, table = S.segment(sc["ndsm"], sc["unit"], sc["origin"], connectivity=8, **params)
    label4, table4 = S.segment(sc["ndsm"], sc["unit"], sc["origin"], connectivity=4, **params)
    kept, corner = [], []
    for b, (i, j, h, w, up) in enumerate(S.LARGE["buildings"], 1):
        m = sc["building"] == b
        assert m.sum() == h * w
        if b == sc["wide"]:
            assert (label[m] == 0).all()                                         # wider than max_window: terrain to the filter
            continue
        if h * w < need:
            assert (label[m] == 0).all() and (label4[m] == 0).all(), b           # the 3 x 3 building: 9 cells
            continue
        ids = np.unique(label[m])
        assert len(ids) == 1 and ids[0] > 0, b                                   # one object, the whole footprint
        if (i, j, h, w, up) in S.CORNER_PAIR:
            corner.append(b)
            continue
        kept.append(b)
        row = int(ids[0]) - 1
        assert table["cells"][row] == h * w == (label == ids[0]).sum(), b
        assert (table["i0"][row], table["i1"][row], table["j0"][row], table["j1"][row]) == (i, i + h - 1, j, j + w - 1)
        assert table["area"][row] == h * w * 0.25 and up - 1.0 < table["height_mean"][row] < up + 1.0 <= table["height_max"][row] + 2.0
        assert abs(table["volume"][row] - up * h * w * 0.25) < 0.15 * up * h * w * 0.25
        assert table["x"][row] == sc["origin"][0] + (j + (w - 1) / 2.0 + 0.5) * 0.5
        assert table["y"][row] == sc["origin"][1] - (i + (h - 1) / 2.0 + 0.5) * 0.5
        assert (label4 == label4[i, j]).sum() == h * w
    assert len(kept) == 5 and len(corner) == 2
    # trees and spikes are foreground but below min_area: dropped; nothing else is labelled
    small = sc["object"] & (sc["building"] == 0)
    fg = S.foreground(sc["ndsm"], sc["unit"], 2.0)
    assert small.sum() == 50 and fg[small].all() and (label[small] == 0).all() and not fg[~sc["object"]].any()
    # the two buildings that touch only at a corner: one object under 8, two under 4
    a, b = (sc["building"] == c for c in corner)
    assert label[a][0] == label[b][0] and table["cells"][label[a][0] - 1] == 128
    assert label4[a][0] != label4[b][0] and table4["cells"][label4[a][0] - 1] == 64 == table4["cells"][label4[b][0] - 1]
    assert table["id"].shape[0] == 6 and table4["id"].shape[0] == 7
    assert table["id"].tolist() == list(range(1, 7)) and (np.diff([np.flatnonzero(label.ravel() == k)[0] for k in range(1, 7)]) > 0).all()


def test_scene_opening_strikes_what_is_narrow(large):
    sc = large
    # open 1.0 on 0.5 units: radius 2, a 5 x 5 window: the 3 x 3 trees, the spikes and the 3 x 3 building go, the others stay whole
    opened = S.foreground(sc["ndsm"], sc["unit"], 2.0, 1.0)
    plain = S.foreground(sc["ndsm"], sc["unit"], 2.0)
    small = sc["object"] & (sc["building"] == 0)
    assert not opened[small].any() and not opened[sc["building"] == 1].any() and not (opened & ~plain).any()
    for b in range(2, sc["wide"]):
        assert opened[sc["building"] == b].all(), b


# ----------------------------------------------------------------------------------------
# the Python layer without a GPU
# ----------------------------------------------------------------------------------------
def test_the_library_exports_the_objects_entry_points():
    names = ("d3d_objects_scratch_bytes", "d3d_objects_foreground", "d3d_objects_label", "d3d_objects_roots", "d3d_objects_stats",
             "d3d_objects_relabel")
    assert all(n in _lib.SIGNATURES for n in names)
    assert _lib.ABI_VERSION == 11 and objects.TILE == 64 and objects.SLOTS == 9
    lib = _lib.load()
    assert lib.d3d_objects_scratch_bytes(100, 50) >= 100 * 50 * 4
    assert lib.d3d_objects_scratch_bytes(0, 5) == 0 and lib.d3d_objects_scratch_bytes(1 << 16, 1 << 15) == 0
    assert lib.d3d_objects_scratch_bytes((1 << 31) - 1, 1) == 0 and lib.d3d_objects_scratch_bytes((1 << 31) - 2, 1) > 0


def test_argument_errors_need_no_gpu():
    g = _grid(1.0, 1.0, 6, 4)
    ok = torch.zeros(4, 6)
    for call in (lambda: objects.segment(ok, g), lambda: objects.foreground(ok, g), lambda: objects.label_components(ok > 0),
                 lambda: objects.label_components(torch.zeros(4, 6, dtype=torch.uint8), 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (torch.zeros(4, 6, dtype=torch.float64), torch.zeros(24), torch.zeros(1, 4, 6), torch.zeros(4, 6, dtype=torch.int32)):
        with pytest.raises(ValueError):
            objects.segment(bad, g)
        with pytest.raises(ValueError):
            objects.label_components(bad)
    with pytest.raises(ValueError, match="does not match the grid"):
        objects.segment(torch.zeros(6, 4), g)
    with pytest.raises(ValueError, match="connectivity"):
        objects.label_components(ok > 0, 6)
    with pytest.raises(ValueError, match="min_height"):
        objects.segment(ok, g, min_height=-1.0)
    with pytest.raises(ValueError, match="outside 1..1024"):
        objects.segment(ok, g, open=0.2)                                          # a radius of 0 cells, before the device check
    with pytest.raises(TypeError):
        objects.segment(ok, "grid")
    with pytest.raises(TypeError):
        objects.label_components(np.zeros((4, 6), bool))
    for s in ({}, {"path": "o.tiff"}, {"path": "o.tif", "table": "o.txt"}, {"path": "o.tif", "table": 3}, {"path": "o.tif", "connectivity": 5}):
        with pytest.raises(ValueError):
            objects.check_settings(s)
    assert objects.check_settings({"path": "o.tif", "table": "o.csv", "min_area": 4}) == (2.0, 4.0, 8, 0.0)


def test_csv_bytes_and_label_raster():
    h = np.full((4, 5), np.nan, np.float32)
    h[0, 0:3] = [2.0, 3.5, 2.25]
    h[2, 4] = 9.0
    label, t = S.segment(h, (0.5, 2.0), (10.0, 100.0), min_area=0.0, connectivity=4)
    want = ("id,cells,area,x,y,i0,i1,j0,j1,height_max,height_mean,volume\n"
            "1,3,3.0,10.75,99.0,0,0,0,2,3.5,2.5833333333333335,7.75\n"
            "2,1,1.0,12.25,95.0,2,2,4,4,9.0,9.0,9.0\n")
    assert objects.csv_bytes(t) == want.encode("ascii") == S.csv_text(t).encode("ascii")
    assert objects.csv_bytes({c: np.zeros(0, np.int64 if c in ("id", "cells", "i0", "i1", "j0", "j1") else np.float64) for c in S.COLUMNS}) \
        == b"id,cells,area,x,y,i0,i1,j0,j1,height_max,height_mean,volume\n"
    r = objects.label_raster(label, h)
    assert r.dtype == np.float32 and np.isnan(r[1, 1]) and r[0, 0] == 1.0 and r[2, 4] == 2.0 and np.isnan(r).sum() == 16
    with pytest.raises(ValueError, match="2\\^24"):
        objects.label_raster(np.full((1, 1), (1 << 24) + 1, np.int32), np.zeros((1, 1), np.float32))
    # the table of the package from the same integers is the restatement's
    ids, s = S.statistics(h, S.roots(S.foreground(h, (0.5, 2.0)), 4))
    acc = np.stack([s[k] for k in ("cells", "sum_i", "sum_j", "hsum", "i0", "i1", "j0", "j1", "hmax")], 1)
    grid = DsmGrid([10.0, 12.5, 92.0, 100.0], [0.5, 2.0], size=(5, 4))
    assert S.same_table(objects.table_of(acc, grid, 1), t)


def test_cli_flags():
    a = objects.parser().parse_args(["--ndsm", "n.tif", "--out", "o.tif"])
    assert objects.settings_from_args(a, a.out) == {"path": "o.tif", "table": None, "min_height": 2.0, "min_area": 10.0, "connectivity": 8,
                                                    "open": 0.0, "nodata": -9999.0}
    b = objects.parser().parse_args(["--ndsm", "n.tif", "--out", "o.tif", "--table", "o.csv", "--min_height", "1.5", "--min_area", "4",
                                     "--connectivity", "4", "--open", "0.5", "--nodata", "0"])
    assert objects.settings_from_args(b, b.out) == {"path": "o.tif", "table": "o.csv", "min_height": 1.5, "min_area": 4.0, "connectivity": 4,
                                                    "open": 0.5, "nodata": 0.0}
    for argv in (["--out", "o.tif"], ["--ndsm", "n.tif"], ["--ndsm", "n.tif", "--out", "o.png"],
                 ["--ndsm", "n.tif", "--out", "o.tif", "--connectivity", "6"], ["--ndsm", "n.tif", "--out", "o.tif", "--min_height", "-1"],
                 ["--ndsm", "n.tif", "--out", "o.tif", "--table", "o.txt"]):
        with pytest.raises(SystemExit):
            objects.main(argv)


def test_predict_objects_flags_are_off_by_default_and_need_dtm():
    a = predict.parse_args(["--output_folder", "o"])
    assert a.objects is None and a.objects_table is None
    assert (a.objects_min_height, a.objects_min_area, a.objects_connectivity, a.objects_open) == (2.0, 10.0, 8, 0.0)
    base = ["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0,1", "--dsm_nodata", "-1"]
    for source in (["--dsm_source", "pc"], ["--dsm_source", "mesh", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1", "--mesh_voxel", "0.1"]):
        b = predict.parse_args(base + ["--dtm", "t.tif", "--objects", "o.tif", "--objects_table", "o.csv", "--objects_min_height", "3",
                                       "--objects_min_area", "20", "--objects_connectivity", "4", "--objects_open", "0.3"] + source)
        assert predict._objects_settings(b) == {"path": "o.tif", "table": "o.csv", "min_height": 3.0, "min_area": 20.0, "connectivity": 4,
                                                "open": 0.3, "nodata": -1.0}
    with pytest.raises(SystemExit):
        predict.parse_args(base + ["--objects", "o.tif"])                                         # no --dtm
    with pytest.raises(SystemExit):
        predict.parse_args(base + ["--dtm", "t.tif", "--objects", "o.tif", "--objects_connectivity", "5"])


def test_predict_and_fuse_refuses_objects_without_dtm():
    from deep3d_aerial_amd import pipeline

    with pytest.raises(ValueError, match="objects needs dtm"):
        pipeline.predict_and_fuse(None, [], "o", dsm={"path": "d.tif", "border": [0, 1, 0, 1]}, objects={"path": "o.tif"})
    with pytest.raises(ValueError, match="connectivity"):
        pipeline.predict_and_fuse(None, [], "o", dsm={"path": "d.tif", "border": [0, 1, 0, 1]}, dtm={"path": "t.tif"},
                                  objects={"path": "o.tif", "connectivity": 3})
