"""Bare-earth terrain model (DTM) and object heights (nDSM) from the DSM.

The reference has no DTM; the rule is this project's, in the manner of the DSM's (dsm.py): every step is exact or rounded once
at a stated place, so every output is the same bits run to run and equals a direct numpy restatement (tests/dtm_scene.py).

* Input.  height [H,W] fp32, NaN where empty, on a DsmGrid with units (ux, uy).
* Parameters (choices of this project, not measurements): max_window 40.0 (world units: the widest object removed),
  slope 0.3, dh0 0.3, dh_max 2.5.  All finite; max_window > 0, slope >= 0, 0 <= dh0 <= dh_max.
* Levels.  A progressive morphological filter.  With u = max(ux, uy), level k = 1..K has the world half-width
  a_k = 2^(k-1) u (a_0 = 0), the cell radii rx_k = max(1, floor(a_k / ux + 0.5)) and ry_k alike (fp64), and the threshold
  dh_k = fp32(min(dh_max, dh0 + 2 slope (a_k - a_(k-1)))), computed in fp64 and rounded once.  K is the smallest k with
  2 a_k + u >= max_window.  A radius above D3D_DTM_MAX_RADIUS (1024) is a ValueError before any launch.
* Erosion.  erode(s, rx, ry)[i,j] is the smallest non-NaN value of s in rows i-ry..i+ry and columns j-rx..j+rx, clipped to
  the raster, in the IEEE total order (-0.0 < +0.0, the DSM's height key); NaN when the window holds no value.  dilate is the
  same with the largest value; open = dilate(erode(.)).  Both are exact selections, so the result depends on no tile size,
  segment length or launch shape.  Every NaN written is 0x7fc00000.
* One level.  With s_0 = height: o_k = open(s_(k-1), rx_k, ry_k); a cell is struck at level k when its input is not NaN, it
  has not been struck before and fp32(s_(k-1) - o_k) > dh_k; s_k = o_k everywhere.  level [H,W] uint8: 0 for ground, k for
  the level that struck the cell, 255 where the input is empty.
* DTM.  ground = height where level == 0, else NaN.  The DTM is ground with every NaN cell filled by a pull-push pyramid:
  level 0 is ground, level l+1 has size ceil(W_l / 2) x ceil(H_l / 2), down to 1 x 1.
  Pull: a parent (I, J) is the mean of its non-NaN children (2I+a, 2J+b) in range, summed in fp64 in the order
  (a, b) = (0,0), (0,1), (1,0), (1,1), divided by their number and rounded once to fp32; NaN when it has none.
  Push, from the top level down: a cell (i, j) of level l that is still NaN gets fp32(sum(w v) / sum(w)), in fp64, over up to
  four parents, those of a bilinear tap at the cell centre: I0 = i >> 1, I1 = I0 + (i & 1 ? 1 : -1), J alike; weights
  9 (I0,J0), 3 (I0,J1), 3 (I1,J0), 1 (I1,J1), taken in that order.  Parents out of range are skipped (so are NaN parents, which
  exist only when no cell has a value).  Cells that held a value are never changed.  With no ground cell the DTM is all NaN.
* nDSM.  ndsm = fp32(height - dtm), NaN where height is NaN.
* Determinism.  No float atomics anywhere (there is no atomic at all).
* Files.  DTM, nDSM and level are written by dsm.write_dsm (float32 GeoTIFF + .tfw, the DSM's grid and nodata); the level
  raster holds 0..K as float32 with nodata where the input is empty, so dsm.read_dsm reads all three back.

The opening is two running-extreme passes per direction (van Herk / Gil-Werman on height keys, csrc/dtm.hip): its work and its
bytes per cell do not depend on the radius.  Classification, pull, push, ground mask and nDSM are one kernel each.

    python -m deep3d_aerial_amd.dtm --dsm D.tif --out T.tif [--ndsm N.tif] [--ground G.tif] [--max_window 40] [--slope 0.3]
        [--dh0 0.3] [--dh_max 2.5] [--nodata -9999]
"""
import argparse
import math

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .dsm import DsmGrid, check_grid, read_dsm, write_dsm

MAX_RADIUS = _lib.CONSTANTS["D3D_DTM_MAX_RADIUS"]
DEFAULTS = {"max_window": 40.0, "slope": 0.3, "dh0": 0.3, "dh_max": 2.5}   # choices, not measurements
MAX_LEVELS = 254


def check_params(max_window, slope, dh0, dh_max):
    """The four filter parameters as floats, or ValueError."""
    vals = []
    for name, v in (("max_window", max_window), ("slope", slope), ("dh0", dh0), ("dh_max", dh_max)):
        if not _geom.is_real(v):
            raise ValueError("%s must be a finite number (got %r)" % (name, v))
        vals.append(float(v))
    w, s, d0, d1 = vals
    if not w > 0:
        raise ValueError("max_window must be > 0 (got %g)" % w)
    if not s >= 0:
        raise ValueError("slope must be >= 0 (got %g)" % s)
    if not 0 <= d0 <= d1:
        raise ValueError("0 <= dh0 <= dh_max does not hold (dh0 %g, dh_max %g)" % (d0, d1))
    return w, s, d0, d1


def levels(grid, max_window=DEFAULTS["max_window"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"], dh_max=DEFAULTS["dh_max"]):
    """The host table [(rx, ry, dh)] of the levels 1..K (module docstring): ints and an fp32 threshold as a Python float."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    w, s, d0, d1 = check_params(max_window, slope, dh0, dh_max)
    ux, uy = grid.unit
    u = max(ux, uy)
    table, a_prev, k = [], 0.0, 1
    while True:
        a = 2.0 ** (k - 1) * u
        rx = max(1, int(math.floor(a / ux + 0.5)))
        ry = max(1, int(math.floor(a / uy + 0.5)))
        if rx > MAX_RADIUS or ry > MAX_RADIUS:
            raise ValueError("level %d needs the radius (%d, %d) cells: above %d (max_window %g on units %g, %g)"
                             % (k, rx, ry, MAX_RADIUS, w, ux, uy))
        table.append((rx, ry, float(np.float32(min(d1, d0 + 2.0 * s * (a - a_prev))))))
        if 2.0 * a + u >= w:
            return table
        if k == MAX_LEVELS:
            raise ValueError("more than %d levels" % MAX_LEVELS)
        a_prev, k = a, k + 1


def _raster(t, name):
    return _geom.check_raster(t, name, (torch.float32,), 1 << 31, "2^31", "the terrain filter runs")


def _radius(rx, ry):
    for r in (rx, ry):
        if not _geom.is_int(r, 1, MAX_RADIUS):
            raise ValueError("radius %r outside 1..%d" % (r, MAX_RADIUS))
    return int(rx), int(ry)


def _morph(name, height, rx, ry, out=None, scratch=None):
    rx, ry = _radius(rx, ry)
    H, W = _raster(height, "height")
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(height)
    if scratch is None:
        scratch = _geom.scratch(lib.d3d_dtm_scratch_bytes, W, H, device=height.device)
    _lib.check(getattr(lib, name)(_ptr(height), _ptr(out), W, H, rx, ry, _ptr(scratch[0]), scratch[1], _stream()), name)
    return out


def erode(height, rx, ry):
    """The erosion of an [H,W] fp32 device raster by the (2 rx + 1) x (2 ry + 1) window; a new tensor."""
    return _morph("d3d_dtm_erode", height, rx, ry)


def dilate(height, rx, ry):
    """The dilation, likewise."""
    return _morph("d3d_dtm_dilate", height, rx, ry)


def open_(height, rx, ry):
    """dilate(erode(height)), likewise."""
    return _morph("d3d_dtm_open", height, rx, ry)


def classify_ground(height, grid, max_window=DEFAULTS["max_window"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"],
                    dh_max=DEFAULTS["dh_max"]):
    """(level [H,W] uint8, s_K [H,W] fp32: the last surface) of the level loop; queued on the caller's stream."""
    check_grid(height, grid, "height")
    table = levels(grid, max_window, slope, dh0, dh_max)   # before any launch
    H, W = _raster(height, "height")
    lib = _lib.load()
    level = torch.empty((H, W), dtype=torch.uint8, device=height.device)
    surfaces = [torch.empty_like(height), torch.empty_like(height)]
    scratch = _geom.scratch(lib.d3d_dtm_scratch_bytes, W, H, device=height.device)
    s = height
    for k, (rx, ry, dh) in enumerate(table, 1):
        o = _morph("d3d_dtm_open", s, rx, ry, out=surfaces[k % 2], scratch=scratch)
        _lib.check(lib.d3d_dtm_classify(_ptr(s), _ptr(o), dh, k, _ptr(level), W, H, _stream()), "d3d_dtm_classify")
        s = o
    return level, s


def fill_pull_push(raster):
    """The pull-push fill of an [H,W] fp32 device raster (NaN = empty); a new tensor, the input is not changed."""
    H, W = _raster(raster, "raster")
    lib = _lib.load()
    out = torch.empty_like(raster)
    out.copy_(raster)
    pyramid = [out]
    while pyramid[-1].shape != (1, 1):
        h, w = pyramid[-1].shape
        coarse = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=raster.device)
        _lib.check(lib.d3d_dtm_pull(_ptr(pyramid[-1]), w, h, _ptr(coarse), _stream()), "d3d_dtm_pull")
        pyramid.append(coarse)
    for fine, coarse in zip(pyramid[-2::-1], pyramid[:0:-1]):
        _lib.check(lib.d3d_dtm_push(_ptr(coarse), _ptr(fine), int(fine.shape[1]), int(fine.shape[0]), _stream()), "d3d_dtm_push")
    return out


def dsm_to_dtm(height, grid, max_window=DEFAULTS["max_window"], slope=DEFAULTS["slope"], dh0=DEFAULTS["dh0"],
               dh_max=DEFAULTS["dh_max"]):
    """height [H,W] fp32 device raster on `grid` -> (dtm [H,W] fp32, level [H,W] uint8, ndsm [H,W] fp32), queued on the caller's
    stream.  CPU tensors are refused."""
    level, _ = classify_ground(height, grid, max_window, slope, dh0, dh_max)
    H, W = grid.shape
    lib = _lib.load()
    ground = torch.empty_like(height)
    _lib.check(lib.d3d_dtm_ground(_ptr(height), _ptr(level), _ptr(ground), W, H, _stream()), "d3d_dtm_ground")
    dtm = fill_pull_push(ground)
    ndsm = torch.empty_like(height)
    _lib.check(lib.d3d_dtm_ndsm(_ptr(height), _ptr(dtm), _ptr(ndsm), W, H, _stream()), "d3d_dtm_ndsm")
    return dtm, level, ndsm


# ----------------------------------------------------------------------------------------
# files, settings, CLI
# ----------------------------------------------------------------------------------------
def check_settings(settings):
    """The settings of build_and_write, checked without a GPU: {"path"} and optionally {"ndsm", "ground", "max_window", "slope",
    "dh0", "dh_max", "nodata"}.  Returns the four parameters."""
    for key in ("path", "ndsm", "ground"):
        p = settings.get(key)
        if p is None and key != "path":
            continue
        if not isinstance(p, str) or not p.endswith(".tif"):
            raise ValueError("the DTM setting %r must be a path that ends in .tif (got %r)" % (key, p))
    return check_params(*(settings.get(k, DEFAULTS[k]) for k in ("max_window", "slope", "dh0", "dh_max")))


def build_and_write(height, grid, settings):
    """The DTM of a DSM raster (device tensor, or a host array that is moved to the GPU) with settings {"path", "ndsm", "ground",
    "max_window", "slope", "dh0", "dh_max", "nodata"} -> writes <path> and, when given, the nDSM and the level raster, each
    with its .tfw; returns (dtm, level, ndsm)."""
    params = check_settings(settings)
    if not isinstance(height, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError("the terrain filter runs on the GPU (no CPU fallback)")
        height = torch.from_numpy(np.array(height, np.float32)).cuda()   # (a copy: the array may be read-only)
    dtm, level, ndsm = dsm_to_dtm(height, grid, *params)
    nodata = settings.get("nodata", -9999.0)
    write_dsm(settings["path"], dtm, grid, nodata=nodata)
    if settings.get("ndsm") is not None:
        write_dsm(settings["ndsm"], ndsm, grid, nodata=nodata)
    if settings.get("ground") is not None:
        lv = level.cpu().numpy()
        write_dsm(settings["ground"], np.where(lv == 255, np.float32(np.nan), lv.astype(np.float32)), grid, nodata=nodata)
    return dtm, level, ndsm


def add_arguments(ap, prefix=""):
    """The filter's settings as flags (--<prefix>max_window, ...); used by this module's CLI and by predict (--dtm_*)."""
    ap.add_argument("--%sndsm" % prefix, default=None, help="also write the nDSM (DSM - DTM) to this .tif (+ .tfw)")
    ap.add_argument("--%sground" % prefix, default=None,
                    help="also write the level raster to this .tif: 0 ground, k the level that struck the cell, nodata where empty")
    ap.add_argument("--%smax_window" % prefix, type=float, default=DEFAULTS["max_window"], help="widest object removed, world units")
    ap.add_argument("--%sslope" % prefix, type=float, default=DEFAULTS["slope"], help="terrain slope the thresholds allow for")
    ap.add_argument("--%sdh0" % prefix, type=float, default=DEFAULTS["dh0"], help="height threshold of the first level")
    ap.add_argument("--%sdh_max" % prefix, type=float, default=DEFAULTS["dh_max"], help="largest height threshold")


def settings_from_args(a, path, prefix="", nodata=None):
    g = lambda k: getattr(a, prefix + k)
    return {"path": path, "ndsm": g("ndsm"), "ground": g("ground"), "max_window": g("max_window"), "slope": g("slope"),
            "dh0": g("dh0"), "dh_max": g("dh_max"), "nodata": g("nodata") if nodata is None else nodata}


def check_args(ap, a, path, prefix="", nodata=None):
    """Argument errors of the flags, in the parser's words; returns the settings."""
    s = settings_from_args(a, path, prefix, nodata)
    try:
        check_settings(s)
    except ValueError as e:
        ap.error(str(e))
    return s


def parser():
    ap = argparse.ArgumentParser(description="DTM (bare-earth terrain) and nDSM from a DSM file of this project")
    ap.add_argument("--dsm", required=True, help="DSM file (.tif, as dsm.write_dsm writes it)")
    ap.add_argument("--out", required=True, help="DTM file (.tif; the .tfw is written beside it)")
    add_arguments(ap)
    ap.add_argument("--nodata", type=float, default=-9999.0, help="value written for empty cells")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    settings = check_args(ap, a, a.out)
    if not torch.cuda.is_available():
        raise RuntimeError("the terrain filter runs on the GPU (no CPU fallback)")
    height, grid = read_dsm(a.dsm)
    dtm, level, _ = build_and_write(height, grid, settings)
    ground = int((level == 0).sum())
    print("DTM %s: %d x %d, %d levels, %d ground cells of %d" % (a.out, grid.width, grid.height, len(levels(grid, *check_settings(settings))),
                                                                 ground, int((level != 255).sum())))
    return a.out


if __name__ == "__main__":
    main()
