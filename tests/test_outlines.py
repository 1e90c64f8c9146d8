"""The outlines (deep3d_aerial_amd/outlines.py) without a GPU: the properties of the rule on the serial trace of
tests/outlines_scene.py over every labelling pattern, the refusal of labels that are not connected, a hand-made raster, the file
against a literal, the package's host part against the restatement, the settings and flags, and the header."""
import json
import os
import re

import numpy as np
import pytest
import torch

import objects_scene as OS
import outlines_scene as S
from deep3d_aerial_amd import _lib, objects, outlines, predict
from deep3d_aerial_amd.dsm import DsmGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (7, 9), (33, 31)]


def _cases():
    for shape in SHAPES:
        for name, m in OS.patterns(*shape).items():
            for conn in (4, 8):
                yield shape, name, conn, S.labelled(m, conn)


@pytest.fixture(scope="module")
def traced():
    return [(shape, name, conn, lab, S.trace(lab, conn)) for shape, name, conn, lab in _cases()]


def test_one_outer_ring_per_object_first_and_the_areas_add_up(traced):
    for shape, name, conn, lab, rings in traced:
        polys = S.polygons(rings, conn)
        assert [p["id"] for p in polys] == list(range(1, int(lab.max()) + 1)), (shape, name, conn)
        for p in polys:
            mine = [r for r in rings if r["object"] == p["id"]]
            assert mine[0]["area2"] > 0 and all(r["area2"] < 0 for r in mine[1:]), (shape, name, conn, p["id"])
            assert p["rings"] == mine                                                  # the outer ring comes first in ring order
            assert sum(r["area2"] for r in mine) == 2 * int((lab == p["id"]).sum()), (shape, name, conn, p["id"])
        for r in rings:
            assert r["nh"] % 2 == 0 and r["nv"] % 2 == 0 and r["nh"] + r["nv"] == r["length"] and len(r["vertices"]) >= 4
        assert [r["leader"] for r in rings] == sorted(r["leader"] for r in rings)


def test_filling_the_polygons_gives_the_label_raster_back(traced):
    for shape, name, conn, lab, rings in traced:
        assert np.array_equal(S.fill(S.polygons(rings, conn), lab.shape), lab), (shape, name, conn)


def test_labels_made_under_8_and_outlined_under_4_are_refused():
    grid = DsmGrid([0.0, 9.0, 0.0, 7.0], [1.0, 1.0], size=(9, 7))
    for name in ("diagonal", "checkerboard"):
        lab = S.labelled(OS.patterns(7, 9)[name], 8)
        assert lab.max() == 1
        rings = S.trace(lab, 4)
        with pytest.raises(ValueError, match="object 1 has %d outer rings: not connected under connectivity 4" % len(rings)):
            S.polygons(rings, 4)
        v, start, obj = S.arrays(rings)
        with pytest.raises(ValueError, match="object 1 has %d outer rings: not connected under connectivity 4" % len(rings)):
            outlines.polygons({"vertices": v, "ring_start": start, "ring_object": obj}, grid, 4)
        assert len(S.polygons(S.trace(lab, 8), 8)) == 1


def test_the_hand_made_raster():
    L = S.hand_made()
    for conn in (4, 8):
        rings = S.trace(L, conn)
        polys = S.polygons(rings, conn)
        assert [p["id"] for p in polys] == list(range(1, 10)) and [len(p["rings"]) for p in polys] == [1, 1, 1, 1, 2, 1, 1, 1, 1]
        assert np.array_equal(S.fill(polys, L.shape), L)
        by = {p["id"]: p for p in polys}
        # four labels around the corner (2, 2): each ring passes it once and stays a square
        for k in (1, 2, 3, 4):
            assert (2, 2) in by[k]["rings"][0]["vertices"] and len(by[k]["rings"][0]["vertices"]) == 4 and by[k]["rings"][0]["area2"] == 8
        # 4-adjacent labels share a lattice line, each on its own side of it
        assert by[1]["rings"][0]["vertices"] == [(0, 0), (2, 0), (2, 2), (0, 2)] and by[2]["rings"][0]["vertices"] == [(0, 2), (2, 2), (2, 4), (0, 4)]
        # the hole of 5 is clockwise and object 6 lies inside it
        hole = by[5]["rings"][1]
        assert hole["area2"] == -18 and sorted(hole["vertices"]) == [(2, 7), (2, 10), (5, 7), (5, 10)]
        assert by[6]["rings"][0]["vertices"] == [(3, 8), (4, 8), (4, 9), (3, 9)]
        # the raster's edges
        assert by[5]["rings"][0]["vertices"] == [(0, 6), (7, 6), (7, 11), (0, 11)] and by[7]["rings"][0]["vertices"] == [(8, 0), (9, 0), (9, 5), (8, 5)]
        assert by[8]["rings"][0]["vertices"] == [(5, 0), (7, 0), (7, 1), (5, 1)] and by[9]["rings"][0]["vertices"] == [(8, 10), (9, 10), (9, 11), (8, 11)]
    st = S.trace(S.stripes(), 8)
    assert [len(r["vertices"]) for r in st] == [4] * 6 and [r["object"] for r in st] == [1, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError, match="negative"):
        S.trace(np.array([[1, -1]], np.int32), 8)


def test_the_pinch_is_where_the_connectivities_differ():
    L = np.array([[1, 0], [0, 1]], np.int32)
    r8, r4 = S.trace(L, 8), S.trace(L, 4)
    assert len(r8) == 1 and r8[0]["vertices"].count((1, 1)) == 2 and r8[0]["length"] == 8 and r8[0]["area2"] == 4
    assert len(r4) == 2 and all(r["area2"] == 2 for r in r4)
    hole = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], np.int32)           # the label joins across the hole's corner under 8 only:
    assert [r["area2"] for r in S.trace(hole, 8)] == [16, -2]             # the hole stays a ring of its own
    assert [r["area2"] for r in S.trace(hole, 4)] == [14]                  # under 4 it opens into the outer ring
    closed = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], np.int32)
    assert [r["area2"] for r in S.trace(closed, 8)] == [18, -2]


WANT = (b'{"type":"FeatureCollection","features":[\n'
        b'{"type":"Feature","properties":{"id":1,"rings":2,"vertices":8,"perimeter":20.0},"geometry":{"type":"Polygon","coordinates":'
        b'[[[10.0,100.0],[10.0,94.0],[11.5,94.0],[11.5,100.0],[10.0,100.0]],[[11.0,98.0],[11.0,96.0],[10.5,96.0],[10.5,98.0],[11.0,98.0]]]}},\n'
        b'{"type":"Feature","properties":{"id":3,"rings":1,"vertices":4,"perimeter":5.0},"geometry":{"type":"Polygon","coordinates":'
        b'[[[12.0,96.0],[12.0,94.0],[12.5,94.0],[12.5,96.0],[12.0,96.0]]]}}\n'
        b']}\n')


def _hand_rings():
    """A 3 x 3 ring of label 1 with its hole, and one cell of label 3, as label_outlines returns them (ring order)."""
    v = np.array([[0, 0], [3, 0], [3, 3], [0, 3], [1, 2], [2, 2], [2, 1], [1, 1], [2, 4], [3, 4], [3, 5], [2, 5]], np.int32)
    return {"vertices": v, "ring_start": np.array([0, 4, 8, 12], np.int32), "ring_object": np.array([1, 1, 3], np.int32)}


def test_geojson_bytes_of_hand_written_rings():
    grid = DsmGrid([10.0, 12.5, 94.0, 100.0], [0.5, 2.0], size=(5, 3))
    polys = outlines.polygons(_hand_rings(), grid)
    assert polys["area2"].tolist() == [18, -2, 2] and polys["nh"].tolist() == [6, 2, 2] and polys["nv"].tolist() == [6, 2, 2]
    assert polys["id"].tolist() == [1, 3] and polys["polygon_start"].tolist() == [0, 2, 3] and polys["perimeter"].tolist() == [20.0, 5.0]
    data = outlines.geojson_bytes(polys)
    assert data == WANT
    # the raster of those rings, through the restatement
    L = np.zeros((3, 5), np.int32)
    L[:, :3], L[1, 1], L[2, 4] = 1, 0, 3
    assert data == S.geojson_text(S.polygons(S.trace(L, 8), 8), (0.5, 2.0), (10.0, 100.0)).encode("ascii")
    doc = json.loads(data)
    assert doc["type"] == "FeatureCollection" and [f["properties"]["id"] for f in doc["features"]] == [1, 3]
    for f in doc["features"]:
        assert list(f) == ["type", "properties", "geometry"] and list(f["geometry"]) == ["type", "coordinates"]
        assert all(ring[0] == ring[-1] and len(ring) >= 5 for ring in f["geometry"]["coordinates"])
        assert sum(len(ring) - 1 for ring in f["geometry"]["coordinates"]) == f["properties"]["vertices"]
    # with a table: its other columns follow, in objects.COLUMNS order; rows are found by id
    table = {c: np.array([7, 8, 9], np.int64) if c in ("cells", "i0", "i1", "j0", "j1") else np.array([0.5, 1.5, 2.5]) for c in objects.COLUMNS}
    table["id"] = np.array([1, 2, 3], np.int64)
    doc = json.loads(outlines.geojson_bytes(polys, table))
    assert list(doc["features"][1]["properties"]) == ["id", "rings", "vertices", "perimeter"] + list(objects.COLUMNS[1:])
    assert doc["features"][1]["properties"]["cells"] == 9 and doc["features"][1]["properties"]["volume"] == 2.5
    assert doc["features"][0]["properties"]["cells"] == 7
    assert b'"perimeter":5.0,"cells":9,"area":2.5,' in outlines.geojson_bytes(polys, table)
    with pytest.raises(ValueError, match="no row"):
        outlines.geojson_bytes(polys, {c: v[:2] for c, v in table.items()})
    # no objects
    none = outlines.polygons({"vertices": np.zeros((0, 2), np.int32), "ring_start": np.zeros(1, np.int32), "ring_object": np.zeros(0, np.int32)}, grid)
    assert outlines.geojson_bytes(none) == b'{"type":"FeatureCollection","features":[\n\n]}\n' == S.geojson_text([], (1, 1), (0, 0)).encode()
    assert json.loads(outlines.geojson_bytes(none))["features"] == []


def test_the_host_part_equals_the_restatement(traced):
    for shape, name, conn, lab, rings in traced:
        H, W = shape
        grid = DsmGrid([10.0, 10.0 + W * 0.5, -5.0, -5.0 + H * 0.25], [0.5, 0.25], size=(W, H))
        v, start, obj = S.arrays(rings)
        a2, nh, nv = outlines.ring_numbers(v, start)
        assert a2.tolist() == [r["area2"] for r in rings] and nh.tolist() == [r["nh"] for r in rings] and nv.tolist() == [r["nv"] for r in rings]
        polys = outlines.polygons({"vertices": v, "ring_start": start, "ring_object": obj}, grid, conn)
        want = S.geojson_text(S.polygons(rings, conn), (0.5, 0.25), (10.0, -5.0 + H * 0.25)).encode("ascii")
        assert outlines.geojson_bytes(polys) == want, (shape, name, conn)


def test_argument_errors_and_settings_need_no_gpu(tmp_path):
    ok = torch.zeros(4, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        outlines.label_outlines(ok)
    for bad in (torch.zeros(4, 6), torch.zeros(24, dtype=torch.int32), torch.zeros(1, 4, 6, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int64)):
        with pytest.raises(ValueError):
            outlines.label_outlines(bad)
    with pytest.raises(TypeError):
        outlines.label_outlines(np.zeros((4, 6), np.int32))
    for conn in (6, 0, 8.0, True, None):
        with pytest.raises(ValueError, match="connectivity"):
            outlines.label_outlines(ok, conn)
    with pytest.raises(TypeError):
        outlines.polygons(_hand_rings(), "grid")
    for s in ({}, {"path": "o.json"}, {"path": 3}, {"path": "o.geojson", "connectivity": 5}):
        with pytest.raises(ValueError):
            outlines.check_settings(s)
    assert outlines.check_settings({"path": "o.geojson"}) == 8 and outlines.check_settings({"path": "o.geojson", "connectivity": 4}) == 4
    with pytest.raises(ValueError, match="does not match the grid"):
        outlines.build_and_write(ok, DsmGrid([0.0, 4.0, 0.0, 6.0], [1.0, 1.0], size=(4, 6)), {"path": "o.geojson"})
    # the objects' settings carry the key
    for s in ({"path": "o.tif", "outlines": "o.json"}, {"path": "o.tif", "outlines": 3}):
        with pytest.raises(ValueError, match="geojson"):
            objects.check_settings(s)
    assert objects.check_settings({"path": "o.tif", "outlines": "o.geojson", "connectivity": 4}) == (2.0, 10.0, 4, 0.0)
    assert objects.check_settings({"path": "o.tif", "outlines": None}) == (2.0, 10.0, 8, 0.0)
    # the table file read back
    t = {c: np.array([1, 2], np.int64) if c in ("id", "cells", "i0", "i1", "j0", "j1") else np.array([0.1, 1e-300]) for c in objects.COLUMNS}
    (tmp_path / "t.csv").write_bytes(objects.csv_bytes(t))
    back = outlines.read_table(str(tmp_path / "t.csv"))
    assert OS.same_table(back, t)
    (tmp_path / "bad.csv").write_text("id,cells\n1,2\n")
    with pytest.raises(ValueError, match="header"):
        outlines.read_table(str(tmp_path / "bad.csv"))


def test_cli_flags():
    a = outlines.parser().parse_args(["--labels", "l.tif", "--out", "o.geojson"])
    assert (a.table, a.connectivity) == (None, 8)
    for argv in (["--out", "o.geojson"], ["--labels", "l.tif"], ["--labels", "l.tif", "--out", "o.json"],
                 ["--labels", "l.tif", "--out", "o.geojson", "--connectivity", "6"], ["--labels", "l.tif", "--out", "o.geojson", "--table", "t.txt"]):
        with pytest.raises(SystemExit):
            outlines.main(argv)
    # the objects' own CLI: the key is in the settings only when the flag is given
    a = objects.parser().parse_args(["--ndsm", "n.tif", "--out", "o.tif"])
    assert a.outlines is None and "outlines" not in objects.settings_from_args(a, a.out)
    b = objects.parser().parse_args(["--ndsm", "n.tif", "--out", "o.tif", "--outlines", "o.geojson", "--connectivity", "4"])
    assert objects.settings_from_args(b, b.out) == {"path": "o.tif", "table": None, "min_height": 2.0, "min_area": 10.0, "connectivity": 4,
                                                    "open": 0.0, "nodata": -9999.0, "outlines": "o.geojson"}
    with pytest.raises(SystemExit):
        objects.main(["--ndsm", "n.tif", "--out", "o.tif", "--outlines", "o.json"])


def test_the_pipeline_carries_the_key_and_predicts_flags_stay_as_they_are():
    """predict's parser is pinned flag by flag (tests/golden/predict_flags.json), so --objects_outlines is no flag of predict: the
    outlines are reached through the objects' settings dict, which predict_and_fuse checks, and through the two CLIs."""
    from deep3d_aerial_amd import pipeline, products

    base = ["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0,1", "--dsm_nodata", "-1", "--dtm", "t.tif"]
    a = predict.parse_args(base + ["--objects", "o.tif"])
    assert not hasattr(a, "objects_outlines")
    assert predict._objects_settings(a) == {"path": "o.tif", "table": None, "min_height": 2.0, "min_area": 10.0, "connectivity": 8, "open": 0.0,
                                            "nodata": -1.0}
    with pytest.raises(SystemExit):
        predict.parse_args(base + ["--objects", "o.tif", "--objects_outlines", "o.geojson"])
    with pytest.raises(ValueError, match="geojson"):
        pipeline.predict_and_fuse(None, [], "o", dsm={"path": "d.tif", "border": [0, 1, 0, 1]}, dtm={"path": "t.tif"},
                                  objects={"path": "o.tif", "outlines": "o.shp"})
    with pytest.raises(ValueError, match="objects needs dtm"):
        pipeline.predict_and_fuse(None, [], "o", dsm={"path": "d.tif", "border": [0, 1, 0, 1]}, objects={"path": "o.tif", "outlines": "o.geojson"})
    products.check({"cloud": None, "mesh": None, "dsm": {"path": "d.tif"}, "ortho": None, "dtm": {"path": "t.tif"},
                    "objects": {"path": "o.tif", "outlines": "o.geojson"}, "texture": None})
    assert list(products.report_lines(a, {"objects_s": 1.0}, 1)) == ["rank 0/1: objects o.tif in 1.00 s"]


def test_the_header_declares_the_entry_points_and_the_abi_version():
    names = ("d3d_outlines_scratch_bytes", "d3d_outlines_count", "d3d_outlines_edges", "d3d_outlines_rank", "d3d_outlines_rings",
             "d3d_outlines_place", "d3d_outlines_emit")
    text = open(os.path.join(ROOT, "include", "deep3d_planesweep.h")).read()
    assert all(re.search(r"\b%s\(" % n, text) and n in _lib.SIGNATURES for n in names)
    version = int(re.search(r"^#define D3D_ABI_VERSION (\d+)$", text, re.M).group(1))
    assert version == _lib.ABI_VERSION == _lib.load().d3d_version()
    assert "#define D3D_OUTLINES_MAX_CELLS 536870911" in text and outlines.MAX_CELLS == (1 << 29) - 1
    lib = _lib.load()
    assert lib.d3d_outlines_scratch_bytes(100, 50) > 0 and lib.d3d_outlines_scratch_bytes(0, 5) == 0
    assert lib.d3d_outlines_scratch_bytes((1 << 29) - 1, 1) > 0 and lib.d3d_outlines_scratch_bytes(1 << 29, 1) == 0
    make = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\boutlines\.hip\b", make, re.M) and "-DD3D_OUTLINES_SPLIT" in make
