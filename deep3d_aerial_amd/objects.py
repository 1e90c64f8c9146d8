"""The objects of an nDSM: every building or tree as one labelled region with its area, height and volume.

The reference has no such step; the rule is this project's, in the manner of the DSM's (dsm.py) and the DTM's (dtm.py): every
step is exact or rounded once at a stated place, so every output is the same bits for any launch shape and equals a direct
numpy restatement (tests/objects_scene.py).

* Input.  ndsm [H,W] fp32 device raster, NaN where empty, on a DsmGrid with units (ux, uy).  W * H < 2^31 - 1.
* Parameters (choices of this project, not measurements): min_height 2.0 (world units; finite, >= 0), min_area 10.0 (world units
  squared; finite, >= 0), connectivity 8 (4 or 8), open 0.0 (world units; finite, >= 0; 0 is off).
  min_cells = max(1, ceil(min_area / (ux * uy))), computed in fp64.
* Foreground.  A cell is foreground when its nDSM is finite and ndsm >= fp32(min_height), an ordinary IEEE compare.  With
  open > 0 the mask becomes an fp32 raster (1.0 for foreground, 0.0 for everything else, empty cells included), is opened by the
  terrain filter's opening (dtm.open_: d3d_dtm_open, the window clipped at the raster edge) with the radii
  rx = floor(open / ux + 0.5), ry = floor(open / uy + 0.5) (fp64), each of which must lie in 1 .. D3D_DTM_MAX_RADIUS, else a
  ValueError before any launch; the foreground is where the opened mask equals 1.0 (it holds only 0.0 and 1.0).  This strikes
  what is narrower than 2 r + 1 cells, such as walls and wires.
* Components.  Two foreground cells are joined when they are 4-neighbours or, with connectivity 8, 8-neighbours.  The root of a
  component is its smallest linear index i * W + j: a minimum, so it depends on no order of unions and on no tile size.
* Statistics per component, every one an integer: cells; sum_i, sum_j (int64 sums of the row and column indices); the box i0, i1,
  j0, j1; hmax, the largest nDSM value by the height key (dsm_key: the IEEE order); hsum, the int64 sum of
  q(h) = min(2^32 - 1, floor(fp64(h) * 1024 + 0.5)).  Since h >= 0, 2^31 cells cannot overflow the sum.
* Selection and numbering.  A component is kept when cells >= min_cells.  The kept components get the ids 1 .. N in the order
  of their roots.  label [H,W] int32 holds the id of the cell's component, 0 for background and for cells of dropped components.
* Table.  One row per id, in id order: id, cells, area, x, y, i0, i1, j0, j1, height_max, height_mean, volume, with
  area = cells * ux * uy, height_mean = hsum / (1024 * cells), volume = hsum / 1024 * ux * uy (each product and quotient taken
  left to right), height_max = fp64(hmax), and (x, y) the world position of the centroid (sum_j / cells, sum_i / cells) under
  the cell-centre convention of ortho.py (the centre of cell (i, j) is (Xmin + (j + 0.5) ux, Ymax - (i + 0.5) uy)):
      x = Xmin + (sum_j / cells + 0.5) * ux,    y = Ymax - (sum_i / cells + 0.5) * uy.
  All of these are fp64 on the host, from the exact integers.
* Determinism.  Integer atomics only (atomicMin, atomicMax, atomicAdd): no float is ever added by an atomic.
* Files.  The label raster is written by dsm.write_dsm: float32, 0 for background, nodata where the nDSM is empty, so
  dsm.read_dsm reads it back; more than 2^24 objects (the integers float32 holds exactly) is a ValueError.  The table is written
  as CSV with the header above, integers in decimal and floats by repr, so the file is the same bytes run to run.

The components are found tile by tile in LDS (a wave takes a row of 64 cells: runs from one ballot), merged across tile edges
in the global parent raster by a lock-free find-and-atomicMin loop, and resolved in one pass (csrc/objects.hip).

    python -m deep3d_aerial_amd.objects --ndsm N.tif --out O.tif [--table O.csv] [--min_height 2] [--min_area 10]
        [--connectivity 8] [--open 0] [--nodata -9999] [--outlines O.geojson]
"""
import argparse
import math

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .dsm import DsmGrid, check_grid, read_dsm, write_dsm

TILE = _lib.CONSTANTS["D3D_OBJECTS_TILE"]
SLOTS = _lib.CONSTANTS["D3D_OBJECTS_SLOTS"]
MAX_RADIUS = _lib.CONSTANTS["D3D_DTM_MAX_RADIUS"]
MAX_OBJECTS = 1 << 24
DEFAULTS = {"min_height": 2.0, "min_area": 10.0, "connectivity": 8, "open": 0.0}   # choices, not measurements
COLUMNS = ("id", "cells", "area", "x", "y", "i0", "i1", "j0", "j1", "height_max", "height_mean", "volume")
_INT_COLUMNS = ("id", "cells", "i0", "i1", "j0", "j1")


def check_params(min_height=DEFAULTS["min_height"], min_area=DEFAULTS["min_area"], connectivity=DEFAULTS["connectivity"],
                 open=DEFAULTS["open"]):
    """The four parameters as (float, float, int, float), or ValueError."""
    for name, v in (("min_height", min_height), ("min_area", min_area), ("open", open)):
        if not _geom.is_real(v, at_least=0):
            raise ValueError("%s must be a finite number >= 0 (got %r)" % (name, v))
    if not _geom.is_int(connectivity, 4, 8) or int(connectivity) not in (4, 8):
        raise ValueError("connectivity must be 4 or 8 (got %r)" % (connectivity,))
    return float(min_height), float(min_area), int(connectivity), float(open)


def min_cells(grid, min_area=DEFAULTS["min_area"]):
    """max(1, ceil(min_area / (ux * uy))) in fp64."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    if not _geom.is_real(min_area, at_least=0):
        raise ValueError("min_area must be a finite number >= 0 (got %r)" % (min_area,))
    ux, uy = grid.unit
    return max(1, int(math.ceil(float(min_area) / (ux * uy))))


def open_radii(grid, open):
    """None when the opening is off, else (rx, ry) = floor(open / u + 0.5) per axis; outside 1 .. MAX_RADIUS is a ValueError."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    if not _geom.is_real(open, at_least=0):
        raise ValueError("open must be a finite number >= 0 (got %r)" % (open,))
    if float(open) == 0.0:
        return None
    r = tuple(int(math.floor(float(open) / u + 0.5)) for u in grid.unit)
    if not all(1 <= v <= MAX_RADIUS for v in r):
        raise ValueError("open %g on units (%g, %g) needs the radius (%d, %d) cells: outside 1..%d"
                         % ((open,) + tuple(grid.unit) + r + (MAX_RADIUS,)))
    return r


def _raster(t, name, dtypes=(torch.float32,)):
    return _geom.check_raster(t, name, dtypes, (1 << 31) - 1, "2^31 - 1", "the objects are segmented")


def _opened(ndsm, min_height, radii):
    """The opened fp32 mask (0.0 / 1.0) of the foreground of ndsm."""
    from . import dtm

    H, W = (int(s) for s in ndsm.shape)
    maskf = torch.empty_like(ndsm)
    _lib.check(_lib.load().d3d_objects_foreground(_ptr(ndsm), min_height, None, _ptr(maskf), W, H, _stream()), "d3d_objects_foreground")
    return dtm.open_(maskf, *radii)


def foreground(ndsm, grid, min_height=DEFAULTS["min_height"], open=DEFAULTS["open"]):
    """The foreground of ndsm [H,W] fp32 on `grid` (module docstring) as an [H,W] uint8 device raster of 0 and 1."""
    check_grid(ndsm, grid, "ndsm")
    min_height, _, _, open = check_params(min_height=min_height, open=open)
    radii = open_radii(grid, open)   # before any launch
    H, W = _raster(ndsm, "ndsm")
    src, level = (ndsm, min_height) if radii is None else (_opened(ndsm, min_height, radii), 1.0)
    mask = torch.empty((H, W), dtype=torch.uint8, device=ndsm.device)
    _lib.check(_lib.load().d3d_objects_foreground(_ptr(src), level, _ptr(mask), None, W, H, _stream()), "d3d_objects_foreground")
    return mask


def _label(values, level, mask, connectivity, H, W, info=None):
    """parent [H,W] int32 of the fp32 raster `values` thresholded at `level`, or of the uint8 / bool raster `mask`."""
    lib = _lib.load()
    device = (values if mask is None else mask).device
    parent = torch.empty((H, W), dtype=torch.int32, device=device)
    counters = torch.empty((2,), dtype=torch.int64, device=device) if info is not None else None
    _lib.check(lib.d3d_objects_label(_ptr(values), level, _ptr(mask), connectivity, _ptr(parent), W, H, _ptr(counters), _stream()),
               "d3d_objects_label")
    if info is not None:
        info["hooks"], info["repeats"] = (int(v) for v in counters.cpu())
    return parent


def label_components(mask, connectivity=DEFAULTS["connectivity"], info=None):
    """mask [H,W] uint8 or bool device raster (nonzero = foreground) -> the root-index raster [H,W] int32: the smallest linear
    index i * W + j of the cell's component, -1 for background.  info: a dict that receives the border merge's counters."""
    _, _, connectivity, _ = check_params(connectivity=connectivity)
    H, W = _raster(mask, "mask", (torch.uint8, torch.bool))
    return _label(None, 0.0, mask, connectivity, H, W, info)


def _unkey(k):
    """The fp32 value of a height key (geom_shared.h dsm_unkey), as fp64."""
    k = np.asarray(k, np.int64).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32).astype(np.float64)


def table_of(acc, grid, cells_at_least):
    """The table (module docstring) of the statistics acc [n, SLOTS] int64 (host) of the components in root order."""
    acc = np.asarray(acc, np.int64).reshape(-1, SLOTS)
    acc = acc[acc[:, 0] >= cells_at_least]
    ux, uy = grid.unit
    cells = acc[:, 0].astype(np.float64)
    hsum = acc[:, 3].astype(np.float64)
    t = {"id": np.arange(1, acc.shape[0] + 1, dtype=np.int64), "cells": acc[:, 0].copy(), "area": cells * ux * uy,
         "x": grid.x_min + (acc[:, 2].astype(np.float64) / cells + 0.5) * ux,
         "y": grid.y_max - (acc[:, 1].astype(np.float64) / cells + 0.5) * uy,
         "i0": acc[:, 4].copy(), "i1": acc[:, 5].copy(), "j0": acc[:, 6].copy(), "j1": acc[:, 7].copy(),
         "height_max": _unkey(acc[:, 8]), "height_mean": hsum / (1024.0 * cells), "volume": hsum / 1024.0 * ux * uy}
    return {k: t[k] for k in COLUMNS}


def segment(ndsm, grid, min_height=DEFAULTS["min_height"], min_area=DEFAULTS["min_area"], connectivity=DEFAULTS["connectivity"],
            open=DEFAULTS["open"], info=None):
    """ndsm [H,W] fp32 device raster on `grid` -> (label [H,W] int32 device raster, table: a dict of host arrays, one per
    column of COLUMNS).  CPU tensors are refused.  One host read of the number of components sizes the statistics; info (a
    dict) receives "components", "objects" and the border merge's "hooks" and "repeats"."""
    check_grid(ndsm, grid, "ndsm")
    min_height, min_area, connectivity, open = check_params(min_height, min_area, connectivity, open)
    need = min_cells(grid, min_area)
    radii = open_radii(grid, open)   # before any launch
    H, W = _raster(ndsm, "ndsm")
    lib = _lib.load()
    dev = ndsm.device
    if radii is None:
        parent = _label(ndsm, min_height, None, connectivity, H, W, info)
    else:
        parent = _label(_opened(ndsm, min_height, radii), 1.0, None, connectivity, H, W, info)
    scratch = _geom.scratch(lib.d3d_objects_scratch_bytes, W, H, device=dev)
    count = torch.empty((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_objects_roots(_ptr(parent), W, H, _ptr(scratch[0]), scratch[1], _ptr(count[0:1]), _stream()), "d3d_objects_roots")
    n_roots = int(count[0])
    acc = torch.empty((max(n_roots, 1), SLOTS), dtype=torch.int64, device=dev)
    final_id = torch.empty((max(n_roots, 1),), dtype=torch.int32, device=dev)
    label = torch.empty((H, W), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_objects_stats(_ptr(ndsm), _ptr(parent), W, H, _ptr(scratch[0]), scratch[1], n_roots, _ptr(acc), _stream()),
               "d3d_objects_stats")
    _lib.check(lib.d3d_objects_relabel(_ptr(parent), _ptr(acc), n_roots, need, _ptr(final_id), _ptr(label), W, H, _ptr(scratch[0]),
                                       scratch[1], _ptr(count[1:2]), _stream()), "d3d_objects_relabel")
    table = table_of(acc[:n_roots].cpu().numpy(), grid, need)
    n_kept = int(count[1])
    if n_kept != table["id"].shape[0]:
        raise RuntimeError("the label raster has %d objects, the table %d" % (n_kept, table["id"].shape[0]))
    if info is not None:
        info.update(components=n_roots, objects=n_kept)
    return label, table


# ----------------------------------------------------------------------------------------
# files, settings, CLI
# ----------------------------------------------------------------------------------------
def csv_bytes(table):
    """The table as CSV: the header, then one row per object; integers in decimal, floats by repr."""
    lines = [",".join(COLUMNS)]
    for r in range(int(np.asarray(table["id"]).shape[0])):
        lines.append(",".join(str(int(table[c][r])) if c in _INT_COLUMNS else repr(float(table[c][r])) for c in COLUMNS))
    return ("\n".join(lines) + "\n").encode("ascii")


def label_raster(label, ndsm):
    """The label raster as it is written: float32, 0 for background, NaN where the nDSM is empty (host arrays)."""
    label, ndsm = _geom.host(label), _geom.host(ndsm)
    if label.size and int(label.max()) > MAX_OBJECTS:
        raise ValueError("%d objects: float32 holds the ids exactly only up to 2^24" % int(label.max()))
    return np.where(np.isnan(ndsm), np.float32(np.nan), label.astype(np.float32)).astype(np.float32)


def check_settings(settings):
    """The settings of build_and_write, checked without a GPU: {"path"} and optionally {"table", "min_height", "min_area",
    "connectivity", "open", "nodata", "outlines"}.  Returns the four parameters."""
    p = settings.get("path")
    if not isinstance(p, str) or not p.endswith(".tif"):
        raise ValueError("the objects setting 'path' must be a path that ends in .tif (got %r)" % (p,))
    t = settings.get("table")
    if t is not None and (not isinstance(t, str) or not t.endswith(".csv")):
        raise ValueError("the objects setting 'table' must be a path that ends in .csv (got %r)" % (t,))
    params = check_params(*(settings.get(k, DEFAULTS[k]) for k in ("min_height", "min_area", "connectivity", "open")))
    if settings.get("outlines") is not None:
        from . import outlines

        outlines.check_settings({"path": settings["outlines"], "connectivity": params[2]})
    return params


def build_and_write(ndsm, grid, settings, timings=None):
    """The objects of an nDSM raster (device tensor, or a host array that is moved to the GPU) with settings {"path", "table",
    "min_height", "min_area", "connectivity", "open", "nodata", "outlines"} -> writes the label raster <path> with its .tfw and,
    when given, the table and the outlines (outlines.py: the polygons of the label raster as GeoJSON, with the table's columns
    as properties; timings, a dict, gets objects_outlines_s); returns (label, table)."""
    params = check_settings(settings)
    if not isinstance(ndsm, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError("the objects are segmented on the GPU (no CPU fallback)")
        ndsm = torch.from_numpy(np.array(ndsm, np.float32)).cuda()   # (a copy: the array may be read-only)
    label, table = segment(ndsm, grid, *params)
    write_dsm(settings["path"], label_raster(label, ndsm), grid, nodata=settings.get("nodata", -9999.0))
    if settings.get("table") is not None:
        _geom.write_bytes(settings["table"], csv_bytes(table))
    if settings.get("outlines") is not None:
        from . import outlines

        with _geom.timed(timings, "objects_outlines_s"):
            outlines.build_and_write(label, grid, {"path": settings["outlines"], "connectivity": params[2]}, table=table)
    return label, table


def add_arguments(ap, prefix="", outlines=False):
    """The settings as flags (--<prefix>table, ...); used by this module's CLI and by predict (--objects_*).  outlines: also
    --<prefix>outlines; this module's CLI asks for it, predict does not (its flags are the ones of tests/golden/predict_flags.json)."""
    ap.add_argument("--%stable" % prefix, default=None, help="also write the table of the objects to this .csv")
    ap.add_argument("--%smin_height" % prefix, type=float, default=DEFAULTS["min_height"], help="a cell is foreground at this nDSM height, world units")
    ap.add_argument("--%smin_area" % prefix, type=float, default=DEFAULTS["min_area"], help="smallest object kept, world units squared")
    ap.add_argument("--%sconnectivity" % prefix, type=int, default=DEFAULTS["connectivity"], help="4 or 8")
    ap.add_argument("--%sopen" % prefix, type=float, default=DEFAULTS["open"],
                    help="open the foreground by this half-width first, world units (0: off)")
    if outlines:
        ap.add_argument("--%soutlines" % prefix, default=None, help="also write the objects' outlines, polygons in world units, to this .geojson")


def settings_from_args(a, path, prefix="", nodata=None):
    g = lambda k: getattr(a, prefix + k)
    s = {"path": path, "table": g("table"), "min_height": g("min_height"), "min_area": g("min_area"),
         "connectivity": g("connectivity"), "open": g("open"), "nodata": g("nodata") if nodata is None else nodata}
    if getattr(a, prefix + "outlines", None) is not None:   # the key is there only when the flag exists and is given
        s["outlines"] = g("outlines")
    return s


def check_args(ap, a, path, prefix="", nodata=None):
    """Argument errors of the flags, in the parser's words; returns the settings."""
    s = settings_from_args(a, path, prefix, nodata)
    try:
        check_settings(s)
    except ValueError as e:
        ap.error(str(e))
    return s


def parser():
    ap = argparse.ArgumentParser(description="Objects (label raster and table) from an nDSM file of this project")
    ap.add_argument("--ndsm", required=True, help="nDSM file (.tif, as dtm --ndsm writes it)")
    ap.add_argument("--out", required=True, help="label raster (.tif; the .tfw is written beside it)")
    add_arguments(ap, outlines=True)
    ap.add_argument("--nodata", type=float, default=-9999.0, help="value written for empty cells")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    settings = check_args(ap, a, a.out)
    if not torch.cuda.is_available():
        raise RuntimeError("the objects are segmented on the GPU (no CPU fallback)")
    ndsm, grid = read_dsm(a.ndsm)
    try:
        open_radii(grid, settings["open"])
    except ValueError as e:
        ap.error(str(e))
    _, table = build_and_write(ndsm, grid, settings)
    n = int(table["id"].shape[0])
    print("objects %s: %d x %d, %d objects, %d cells, volume %r" % (a.out, grid.width, grid.height, n, int(table["cells"].sum()),
                                                                   float(table["volume"].sum())))
    return a.out


if __name__ == "__main__":
    main()
