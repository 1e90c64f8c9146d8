"""The outlines of the objects: every object of a label raster as a polygon with its holes, written as GeoJSON.

The reference has no such step; the rule is this project's, in the manner of the objects' (objects.py): every step is exact, so
every output is the same bits for any launch shape and equals a plain restatement, a serial trace (tests/outlines_scene.py).

* Input.  label [H,W] int32 device raster: 0 is background, ids > 0 are objects, a negative value is a ValueError.
  1 <= W * H <= 2^29 - 1 (D3D_OUTLINES_MAX_CELLS), so there are fewer than 2^31 unit edges.  connectivity is 4 or 8, the one the
  labels were made with.  Cells outside the raster count as label 0.
* Edges.  Lattice corner (i, j), 0 <= i <= H and 0 <= j <= W, is the upper-left corner of cell (i, j).  For every cell c with
  label L > 0 and every side s whose neighbour across it does not have label L there is one directed unit edge with the cell on
  its left; the sides go counter-clockwise in world coordinates (y up):
      s  side    from          to            direction
      0  top     (i, j+1)      (i, j)        -j
      1  left    (i, j)        (i+1, j)      +i
      2  bottom  (i+1, j)      (i+1, j+1)    +j
      3  right   (i+1, j+1)    (i, j+1)      -i
  The edges are ordered by (cell linear index i * W + j, s); that order is the edge's slot.
* Successor.  For edge (c, s) with direction d and outward normal o (the neighbour offset of side s), LA = c + d is the cell
  ahead on the left and RA = c + d + o the cell ahead on the right; la = (label(LA) == L), ra = (label(RA) == L).
  Connectivity 8: if ra, turn right onto (RA, s - 1); else if la, go straight onto (LA, s); else turn left onto (c, s + 1).
  Connectivity 4: if not la, turn left; else if not ra, go straight; else turn right.
  The two differ only at a corner where L sits on one diagonal and not on the other: connectivity 8 passes through the pinch,
  connectivity 4 stays on its cell.  Every edge has exactly one successor and one predecessor, so the edges fall into closed
  rings.
* Ring.  Its leader is its smallest slot; rings are ordered by leader.  Dropping collinear lattice vertices, a ring's vertices
  are the heads of its corner edges, in ring order; a corner edge is an edge whose successor has another side number.  The
  sequence starts with the first corner edge at or after the leader.  A ring has at least 4 vertices; it may pass a vertex twice,
  but never an edge twice.
* Ring numbers, integers computed on the host from the vertex list.  area2 is twice the signed area: the shoelace sum
  sum_k (x_k y_k+1 - x_k+1 y_k) over (x, y) = (j, -i) in int64; area2 > 0 is an outer ring (counter-clockwise in the world),
  area2 < 0 a hole, and it is never 0.  nh, nv are the number of unit edges along j and along i.
* Polygon of an object.  Its outer ring, then its holes in ring order.  With labels connected under `connectivity` every object
  has exactly one outer ring, which comes first among its rings, and the area2 of its rings sum to twice its cell count.  An
  object with any other number of outer rings is a ValueError naming the id ("not connected under connectivity c").  RFC 7946's
  orientation (outer counter-clockwise, holes clockwise) holds by construction.
* World coordinates.  x = Xmin + j * ux, y = Ymax - i * uy, fp64 on the host: one product, one sum.
* File.  An ASCII GeoJSON FeatureCollection: the line '{"type":"FeatureCollection","features":[', one Feature per line in id
  order, the lines joined by ',', then the line ']}'; a trailing newline ends the file.  A Feature is
      {"type":"Feature","properties":{...},"geometry":{"type":"Polygon","coordinates":[ring, ...]}}
  with the keys in this order, the separators ',' and ':' and no spaces; a ring is its positions [x,y], closed by repeating the
  first; floats are written by repr, integers in decimal.  properties: id, rings, vertices (of all its rings, the closing
  positions not counted), perimeter = fp64(sum of nh) * ux + fp64(sum of nv) * uy over the object's rings and, when a table is
  given, the table's other columns in objects.COLUMNS order.  The bytes are the same run to run.  The coordinates are the grid's
  world units, as the .tfw of the rasters is: GeoJSON carries no CRS here.

The kernels (csrc/outlines.hip) count the boundary sides of every cell, scan them into slots, write every edge's successor slot,
rank the rings by pointer jumping -- round k: t = nx[e]; if m[t] < m[e] then (m[e], dm[e]) = (m[t], 2^k + dm[t]); nx[e] = nx[t];
the round that changes no m is the last, the first with 2^k >= the longest ring -- and place every edge at
ring start + (len - dm[e]) mod len, len = 1 + dm[successor(leader)].  The host does the rest with numpy.

    python -m deep3d_aerial_amd.outlines --labels O.tif --out O.geojson [--table O.csv] [--connectivity 8]
"""
import argparse
import csv

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .dsm import DsmGrid, check_grid, read_dsm

MAX_CELLS = _lib.CONSTANTS["D3D_OUTLINES_MAX_CELLS"]
STATE_BYTES = 16   # the ranking state of an edge
DEFAULT_CONNECTIVITY = 8
_TABLE_INT = ("id", "cells", "i0", "i1", "j0", "j1")


def check_connectivity(connectivity):
    if not _geom.is_int(connectivity, 4, 8) or int(connectivity) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8 (got %r)" % (connectivity,))
    return int(connectivity)


def _empty(dev):
    return {"vertices": torch.empty((0, 2), dtype=torch.int32, device=dev), "ring_start": torch.zeros((1,), dtype=torch.int32, device=dev),
            "ring_object": torch.empty((0,), dtype=torch.int32, device=dev)}


def label_outlines(label, connectivity=DEFAULT_CONNECTIVITY, info=None):
    """label [H,W] int32 device raster -> {"vertices" [V,2] int32 (i, j), "ring_start" [R+1] int32, "ring_object" [R] int32}
    (device tensors; module docstring).  CPU tensors are refused.  Host reads: the number of edges, one word per round of the
    ranking, the number of rings and of vertices.  info (a dict) receives "edges", "rings" and "rounds"; a dict that holds a
    dict "seconds" gets the phases count, edges, rank and emit timed into it (the device is synchronised between them)."""
    connectivity = check_connectivity(connectivity)
    H, W = _geom.check_raster(label, "label", (torch.int32,), MAX_CELLS + 1, "2^29", "the outlines are traced")
    lib, dev, st = _lib.load(), label.device, _stream()
    seconds = info.get("seconds") if info is not None else None
    timed = lambda key: _geom.timed(seconds, key, start=True, always=False)
    scratch = _geom.scratch(lib.d3d_outlines_scratch_bytes, W, H, device=dev)
    with timed("count"):
        offset = torch.empty((H, W), dtype=torch.int32, device=dev)
        counters = torch.empty((2,), dtype=torch.int64, device=dev)
        _lib.check(lib.d3d_outlines_count(_ptr(label), W, H, _ptr(offset), _ptr(scratch[0]), scratch[1], _ptr(counters), st),
                   "d3d_outlines_count")
        E, negative = (int(v) for v in counters.cpu())
    if negative:
        raise ValueError("label holds a negative value: 0 is background and the ids are > 0")
    if info is not None:
        info.update(edges=E, rings=0, rounds=0)
    if E == 0:
        return _empty(dev)
    with timed("edges"):
        succ = torch.empty((E,), dtype=torch.int32, device=dev)
        key = torch.empty((E,), dtype=torch.int32, device=dev)
        state = [torch.empty((E, STATE_BYTES // 4), dtype=torch.int32, device=dev) for _ in range(2)]
        _lib.check(lib.d3d_outlines_edges(_ptr(label), _ptr(offset), connectivity, W, H, E, _ptr(succ), _ptr(key), _ptr(state[0]), st),
                   "d3d_outlines_edges")
    with timed("rank"):
        changed = torch.empty((1,), dtype=torch.int32, device=dev)
        rounds = 0
        while True:
            if rounds > 30:
                raise RuntimeError("the ranking of %d edges did not settle in 31 rounds" % E)
            _lib.check(lib.d3d_outlines_rank(_ptr(state[rounds & 1]), _ptr(state[1 - (rounds & 1)]), E, rounds, _ptr(changed), st),
                       "d3d_outlines_rank")
            rounds += 1
            if not int(changed[0]):
                break
        ranked = state[rounds & 1]
    with timed("emit"):
        del offset
        ring_id = torch.empty((E,), dtype=torch.int32, device=dev)
        count = torch.empty((2,), dtype=torch.int64, device=dev)
        _lib.check(lib.d3d_outlines_rings(_ptr(ranked), W, H, E, _ptr(ring_id), _ptr(scratch[0]), scratch[1], _ptr(count[0:1]), st),
                   "d3d_outlines_rings")
        R = int(count[0])
        if not 1 <= R <= E // 4:
            raise RuntimeError("%d rings of %d edges" % (R, E))
        ring_len = torch.empty((R,), dtype=torch.int32, device=dev)
        ring_edge = torch.empty((R,), dtype=torch.int32, device=dev)
        ring_object = torch.empty((R,), dtype=torch.int32, device=dev)
        ordered = torch.empty((E,), dtype=torch.int32, device=dev)
        corner = torch.empty((E,), dtype=torch.int32, device=dev)
        _lib.check(lib.d3d_outlines_place(_ptr(label), W, H, _ptr(ranked), _ptr(succ), _ptr(key), _ptr(ring_id), E, R, _ptr(ring_len),
                                          _ptr(ring_edge), _ptr(ring_object), _ptr(ordered), _ptr(corner), _ptr(scratch[0]), scratch[1],
                                          _ptr(count[1:2]), st), "d3d_outlines_place")
        V = int(count[1])
        if not 4 * R <= V <= E:
            raise RuntimeError("%d vertices on %d rings of %d edges" % (V, R, E))
        vertices = torch.empty((V, 2), dtype=torch.int32, device=dev)
        ring_start = torch.empty((R + 1,), dtype=torch.int32, device=dev)
        _lib.check(lib.d3d_outlines_emit(_ptr(ordered), _ptr(corner), _ptr(ring_edge), W, H, E, R, V, _ptr(vertices), _ptr(ring_start), st),
                   "d3d_outlines_emit")
    if info is not None:
        info.update(rings=R, rounds=rounds)
    return {"vertices": vertices, "ring_start": ring_start, "ring_object": ring_object}


# ----------------------------------------------------------------------------------------
# the host part: ring numbers, polygons, text
# ----------------------------------------------------------------------------------------
def ring_numbers(vertices, ring_start):
    """(area2, nh, nv) int64 [R] of rings given as host arrays vertices [V,2] (i, j) and ring_start [R+1] (module docstring)."""
    v = np.asarray(vertices, np.int64).reshape(-1, 2)
    start = np.asarray(ring_start, np.int64)
    R = start.shape[0] - 1
    if R == 0:
        return tuple(np.zeros(0, np.int64) for _ in range(3))
    nxt = np.arange(1, v.shape[0] + 1, dtype=np.int64)
    nxt[start[1:] - 1] = start[:-1]
    x, y = v[:, 1], -v[:, 0]
    sums = lambda a: np.add.reduceat(a, start[:-1])
    return sums(x * y[nxt] - x[nxt] * y), sums(np.abs(x[nxt] - x)), sums(np.abs(y[nxt] - y))


def polygons(rings, grid, connectivity=DEFAULT_CONNECTIVITY):
    """The polygons of label_outlines' rings on `grid`, host arrays: {"id" [N] int64, "polygon_start" [N+1] int64 (into the rings
    below), "ring_start" [R+1] int64 (into the vertices below), "ij" [V,2] int32, "xy" [V,2] float64, "area2", "nh", "nv" [R]
    int64, "perimeter" [N] float64}: the rings regrouped by object in id order, each object's outer ring first and its holes after
    it in ring order.  connectivity only words the error for an object that does not have exactly one outer ring."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    v = _geom.host(rings["vertices"]).astype(np.int32).reshape(-1, 2)
    start = _geom.host(rings["ring_start"]).astype(np.int64)
    obj = _geom.host(rings["ring_object"]).astype(np.int64)
    area2, nh, nv = ring_numbers(v, start)
    if (area2 == 0).any() or (obj <= 0).any():
        raise RuntimeError("a ring without area or without an object")
    ids, first, n_rings = np.unique(obj, return_index=True, return_counts=True)
    outer = np.zeros(ids.shape[0], np.int64)
    np.add.at(outer, np.searchsorted(ids, obj), (area2 > 0).astype(np.int64))
    if (outer != 1).any():
        k = int(np.flatnonzero(outer != 1)[0])
        raise ValueError("object %d has %d outer rings: not connected under connectivity %d" % (ids[k], outer[k], connectivity))
    order = np.lexsort((np.arange(obj.shape[0]), area2 < 0, obj))      # by object, the outer ring first, then ring order
    n = (start[1:] - start[:-1])[order]
    new_start = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    take = np.repeat(start[:-1][order] - new_start[:-1], n) + np.arange(int(n.sum()), dtype=np.int64)
    ij = v[take]
    ux, uy = grid.unit
    xy = np.stack([grid.x_min + ij[:, 1].astype(np.float64) * ux, grid.y_max - ij[:, 0].astype(np.float64) * uy], 1)
    polygon_start = np.concatenate([[0], np.cumsum(n_rings)]).astype(np.int64)
    nh_o, nv_o = (np.add.reduceat(a[order], polygon_start[:-1]) if ids.shape[0] else np.zeros(0, np.int64) for a in (nh, nv))
    return {"id": ids.astype(np.int64), "polygon_start": polygon_start, "ring_start": new_start, "ij": ij, "xy": xy,
            "area2": area2[order], "nh": nh[order], "nv": nv[order], "perimeter": nh_o.astype(np.float64) * ux + nv_o.astype(np.float64) * uy}


def geojson_bytes(polys, table=None):
    """The file of the module docstring for the polygons of polygons(); table: the objects' table (objects.COLUMNS), whose rows
    are found by id."""
    from .objects import COLUMNS

    rows = None
    if table is not None:
        tid = np.asarray(table["id"], np.int64)
        order = np.argsort(tid, kind="stable")
        at = np.searchsorted(tid[order], polys["id"])
        if (at >= tid.shape[0]).any() or (tid[order[np.minimum(at, tid.shape[0] - 1)]] != polys["id"]).any():
            raise ValueError("the table has no row for an object of the label raster")
        rows = order[at]
    xy, ps, rs = polys["xy"].tolist(), polys["polygon_start"].tolist(), polys["ring_start"].tolist()
    lines = []
    for k, oid in enumerate(polys["id"].tolist()):
        props = ['"id":%d' % oid, '"rings":%d' % (ps[k + 1] - ps[k]), '"vertices":%d' % (rs[ps[k + 1]] - rs[ps[k]]),
                 '"perimeter":%r' % float(polys["perimeter"][k])]
        if rows is not None:
            r = int(rows[k])
            props += ['"%s":%s' % (c, str(int(table[c][r])) if c in _TABLE_INT else repr(float(table[c][r]))) for c in COLUMNS[1:]]
        coords = []
        for q in range(ps[k], ps[k + 1]):
            pos = ["[%r,%r]" % (x, y) for x, y in xy[rs[q]:rs[q + 1]]]
            coords.append("[" + ",".join(pos + pos[:1]) + "]")
        lines.append('{"type":"Feature","properties":{%s},"geometry":{"type":"Polygon","coordinates":[%s]}}' % (",".join(props), ",".join(coords)))
    return ('{"type":"FeatureCollection","features":[\n' + ",\n".join(lines) + "\n]}\n").encode("ascii")


# ----------------------------------------------------------------------------------------
# files, settings, CLI
# ----------------------------------------------------------------------------------------
def check_settings(settings):
    """The settings of build_and_write, checked without a GPU: {"path"} and optionally {"connectivity"}.  Returns the
    connectivity."""
    p = settings.get("path")
    if not isinstance(p, str) or not p.endswith(".geojson"):
        raise ValueError("the outlines setting 'path' must be a path that ends in .geojson (got %r)" % (p,))
    return check_connectivity(settings.get("connectivity", DEFAULT_CONNECTIVITY))


def build_and_write(label, grid, settings, table=None, timings=None):
    """The outlines of a label raster (int32 device tensor, or a host array of integers that is moved to the GPU) on `grid` with
    settings {"path", "connectivity"} -> writes the GeoJSON file <path>, with the table's columns as properties when a table is
    given; returns the polygons (polygons()).  timings (a dict) gets outlines_gpu_s and outlines_host_s."""
    connectivity = check_settings(settings)
    if not isinstance(label, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError("the outlines are traced on the GPU (no CPU fallback)")
        label = torch.from_numpy(np.array(label, np.int32)).cuda()
    check_grid(label, grid, "label")
    with _geom.timed(timings, "outlines_gpu_s", always=False):
        rings = label_outlines(label, connectivity)
    with _geom.timed(timings, "outlines_host_s", always=False):
        polys = polygons(rings, grid, connectivity)
        _geom.write_bytes(settings["path"], geojson_bytes(polys, table))
    return polys


def read_table(path):
    """The table objects.csv_bytes wrote, as {column: array}."""
    from .objects import COLUMNS

    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or tuple(rows[0]) != COLUMNS:
        raise ValueError("%s: the header is not %s" % (path, ",".join(COLUMNS)))
    cols = list(zip(*rows[1:])) if len(rows) > 1 else [()] * len(COLUMNS)
    return {c: np.array([int(v) for v in col], np.int64) if c in _TABLE_INT else np.array([float(v) for v in col], np.float64)
            for c, col in zip(COLUMNS, cols)}


def read_labels(path):
    """(label [H,W] int32 host array, grid) of a label raster as objects writes it: NaN (empty) becomes 0."""
    raster, grid = read_dsm(path)
    label = np.where(np.isnan(raster), np.float32(0), raster)
    if (label != np.floor(label)).any():
        raise ValueError("%s: not a label raster (a value is no integer)" % path)
    return label.astype(np.int32), grid


def parser():
    ap = argparse.ArgumentParser(description="Outlines (GeoJSON polygons) of a label raster of this project")
    ap.add_argument("--labels", required=True, help="label raster (.tif, as objects --out writes it)")
    ap.add_argument("--out", required=True, help="the polygons (.geojson, in the grid's world units)")
    ap.add_argument("--table", default=None, help="the objects' table (.csv, as objects --table writes it): its columns become properties")
    ap.add_argument("--connectivity", type=int, default=DEFAULT_CONNECTIVITY, help="4 or 8: the one the labels were made with")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    settings = {"path": a.out, "connectivity": a.connectivity}
    try:
        check_settings(settings)
        if a.table is not None and not a.table.endswith(".csv"):
            raise ValueError("--table must be a path that ends in .csv (got %r)" % (a.table,))
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the outlines are traced on the GPU (no CPU fallback)")
    label, grid = read_labels(a.labels)
    polys = build_and_write(label, grid, settings, table=read_table(a.table) if a.table is not None else None)
    print("outlines %s: %d x %d, %d polygons, %d rings, %d vertices" % (a.out, grid.width, grid.height, polys["id"].shape[0],
                                                                        polys["area2"].shape[0], polys["ij"].shape[0]))
    return a.out


if __name__ == "__main__":
    main()
