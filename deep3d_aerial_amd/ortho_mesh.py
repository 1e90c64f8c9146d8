"""Orthophoto of the textured mesh: the mesh of texture.py seen top-down on a DsmGrid, coloured from its atlas.

The reference's TextureMesh has an orthographic image (nOrthoMapResolution in mesh/config.yaml, --orthographic-image-resolution).
The rule below is this project's own; it does not claim to match OpenMVS.

* Grid and coverage.  The grid is any DsmGrid (border, unit, optional size), independent of the DSM's; cell (i, j) samples its
  centre cx = Xmin + (j + .5) ux, cy = Ymax - (i + .5) uy, row 0 north.  Coverage is exactly the mesh DSM's (dsm.py "DSM from a
  triangle mesh", d3d_dsm_from_mesh in the header; one copy of the code, csrc/dsm_tri.h): the same lexicographic (x, y, z) vertex
  order, the same fp64 edge functions E with the inclusive test (every w >= 0 and W = (w_a + w_b) + w_c > 0), the same rejection
  of degenerate and vertical faces (D 0 or not finite) and of non-finite coordinates, the same cell ranges (the XY box's cells
  with a one-cell margin, clipped), and the same sample z = fp32(((w_a z_a + w_b z_b) + w_c z_c) / W), dropped outside
  [Zmin, Zmax] when the border has Z bounds.
* Texcoords.  texcoord [m,6] fp32 (s, t of the three corners) and texnumber [m] int32 are what texture.texcoords and
  write_textured_ply produce.  They travel with the vertices through the lexicographic sort, so the result does not depend on
  the winding or on which corner comes first.  At a covered centre s = ((w_a s_a + w_b s_b) + w_c s_c) / W in fp64, and t alike.
  The texel position on page k = texnumber is x = s P - 0.5, y = (1 - t) h_k - 0.5, P the page width and h_k the page height:
  the inverse of what texture.texcoords writes.
* Colour.  ortho.py's "Colour" on that page at (x, y): x0 = floor(x) clamped to 0 .. P - 1, fx = x - floor(x),
  x1 = min(x0 + 1, P - 1), y alike, the weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy summed in that order in fp64, each
  channel floor(c + 0.5) clamped to 0..255, alpha 255 (the atlas's own alpha byte is not read).  A face is untextured when its
  three texcoord pairs are equal bit for bit (what texture.texcoords writes for a face no view sees), or its texnumber is
  outside 0 .. n_pages - 1, or a texcoord is not finite.  An untextured face still occludes; its colour word is 0.
* Which face wins.  A cell keeps the largest 64-bit key (zk << 32) | colour word (R in the low byte, alpha in the high one).
  With Z up (the default, the mesh DSM's convention) zk = key(z), the order-preserving fp32 -> uint32 key of the DSM; with
  z_down, zk = ~key(z), so the lowest sample wins: the orthophoto shows the side the cameras are on, and ortho.py already
  allows either sign of Z.  No finite sample has zk == 0 in either mode; key 0 is the empty cell.  Ties in height are coincident
  faces, or shared edges that round alike; they go to the larger colour word, so a textured face beats an untextured one there.
  The raster is a function of the set of (triangle, texcoords, page texels): it never depends on the face order.
* Outputs.  rgba [H,W,4] uint8: (0, 0, 0, 0) in empty cells and where an untextured face is on top.  height [H,W] fp32: the
  winning sample, NaN where empty; with Z up this is dsm.mesh_to_dsm on the same grid, bit for bit.
* Files.  ortho.write_ortho: <name>.tif (RGBA8 GeoTIFF) and <name>.tfw.

Out of scope: supersampling or mip levels when a cell is larger than a texel (the tap is one bilinear sample at the centre),
filling the transparent cells, blending of faces.

The rasteriser is HIP (csrc/ortho_mesh.hip): 64-bit integer atomicMax only, so the rasters are bit-reproducible.

    python -m deep3d_aerial_amd.ortho_mesh --textured T.ply --out O.tif --border Xmin,Xmax,Ymin,Ymax[,Zmin,Zmax] [--unit ux,uy]
        [--size W,H] [--z_down]
"""
import argparse
import os

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .dsm import DsmGrid, parse_border, parse_size, parse_unit

DEFAULT_UNIT = (0.1, 0.1)


def atlas_from_pages(pages, page_size, device):
    """Host RGB8 pages [[H_k, page_size, 3] uint8] -> (atlas [sum H_k, page_size] int32 of packed RGBA8 texels with alpha 255,
    page_row [n_pages + 1] int64), both on `device`: the buffer texture.new_atlas lays out."""
    P = int(page_size)
    pages = [np.asarray(p) for p in pages]
    if not pages:
        raise ValueError("at least one page is needed")
    for k, p in enumerate(pages):
        if p.dtype != np.uint8 or p.ndim != 3 or p.shape[2] != 3 or p.shape[1] != P or p.shape[0] < 1:
            raise ValueError("page %d must be [H, %d, 3] uint8 with H >= 1 (got %s %s)" % (k, P, p.shape, p.dtype))
    rgb = np.concatenate(pages, 0)
    rgba = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], 2)
    atlas = torch.from_numpy(np.ascontiguousarray(rgba).view("<i4").reshape(rgb.shape[0], P)).to(device)
    page_row = np.concatenate([[0], np.cumsum([p.shape[0] for p in pages])]).astype(np.int64)
    return atlas, torch.from_numpy(page_row).to(device)


def mesh_to_ortho(vertices, faces, texcoord, texnumber, atlas, page_row, grid, z_down=False):
    """vertices [n,3] fp32, faces [m,3] int32, texcoord [m,6] fp32, texnumber [m] int32, atlas [rows, P] int32 (packed RGBA8) and
    page_row [n_pages + 1] int64, all on one GPU -> (rgba [H,W,4] uint8, height [H,W] fp32 with NaN for empty cells) by the rule
    of this module's docstring, queued on the caller's stream.  CPU tensors are refused; so are face indices outside 0..n-1 and a
    page_row that does not rise from 0 to the atlas's rows (ValueError before any launch: these checks read back to the host)."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    for name, t in (("vertices", vertices), ("faces", faces), ("texcoord", texcoord), ("texnumber", texnumber), ("atlas", atlas),
                    ("page_row", page_row)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_contiguous():
        raise ValueError("vertices must be a contiguous [n,3] float32 tensor (got %s %s)" % (vertices.dtype, tuple(vertices.shape)))
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise ValueError("faces must be a contiguous [m,3] int32 tensor (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if nv >= 1 << 31 or nf >= 1 << 31:
        raise ValueError("%d vertices, %d faces: at most 2^31 - 1 of each" % (nv, nf))
    if texcoord.dtype != torch.float32 or tuple(texcoord.shape) != (nf, 6) or not texcoord.is_contiguous():
        raise ValueError("texcoord must be a contiguous [%d,6] float32 tensor (got %s %s)" % (nf, texcoord.dtype, tuple(texcoord.shape)))
    if texnumber.dtype != torch.int32 or tuple(texnumber.shape) != (nf,) or not texnumber.is_contiguous():
        raise ValueError("texnumber must be a contiguous [%d] int32 tensor (got %s %s)" % (nf, texnumber.dtype, tuple(texnumber.shape)))
    if atlas.dtype != torch.int32 or atlas.dim() != 2 or atlas.shape[1] < 1 or not atlas.is_contiguous():
        raise ValueError("atlas must be a contiguous [rows, page_width] int32 tensor (got %s %s)" % (atlas.dtype, tuple(atlas.shape)))
    if page_row.dtype != torch.int64 or page_row.dim() != 1 or page_row.shape[0] < 2 or not page_row.is_contiguous():
        raise ValueError("page_row must be a contiguous [n_pages + 1] int64 tensor with n_pages >= 1 (got %s %s)"
                         % (page_row.dtype, tuple(page_row.shape)))
    rows = page_row.tolist()
    if rows[0] != 0 or any(b <= a for a, b in zip(rows, rows[1:])) or rows[-1] != int(atlas.shape[0]):
        raise ValueError("page_row %s must rise from 0 to the atlas's %d rows" % (rows, int(atlas.shape[0])))
    if nf:
        lo, hi = torch.stack([faces.min(), faces.max()]).tolist()
        if lo < 0 or hi >= nv:
            raise ValueError("face indices span %d..%d: outside the %d vertices" % (lo, hi, nv))
    for name, t in (("vertices", vertices), ("faces", faces), ("texcoord", texcoord), ("texnumber", texnumber), ("atlas", atlas),
                    ("page_row", page_row)):
        if not t.is_cuda:
            raise RuntimeError("%s is on %s: the orthophoto of the mesh is built on the GPU (no CPU fallback)" % (name, t.device))
        if t.device != vertices.device:
            raise ValueError("vertices on %s, %s on %s" % (vertices.device, name, t.device))
    H, W = grid.shape
    dev = vertices.device
    lib = _lib.load()
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    height = torch.empty((H, W), dtype=torch.float32, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_ortho_mesh_scratch_bytes, nf, W, H, device=dev)
    rc = lib.d3d_ortho_from_mesh(_ptr(vertices) if nv else None, nv, _ptr(faces) if nf else None, nf, _ptr(texcoord) if nf else None,
                                 _ptr(texnumber) if nf else None, _ptr(atlas), _ptr(page_row), len(rows) - 1, int(atlas.shape[1]),
                                 grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], grid.z_min, grid.z_max, W, H, 1 if z_down else 0,
                                 _ptr(scratch), nbytes, _ptr(rgba), _ptr(height), _stream())
    _lib.check(rc, "d3d_ortho_from_mesh")
    return rgba, height


def summary(rgba, height):
    """{"cells", "coloured", "untextured", "empty"}: the cells with a colour (alpha 255), the covered cells whose top face is
    untextured, and the cells no face covers."""
    covered = torch.isfinite(height)
    coloured = rgba[:, :, 3] != 0
    n = int(height.numel())
    nc, ncol = int(covered.sum()), int((coloured & covered).sum())
    return {"cells": n, "coloured": ncol, "untextured": nc - ncol, "empty": n - nc}


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def check_settings(settings):
    """The settings dict {"path", "border", "unit", "size", "z_down"} checked: (DsmGrid, z_down).  No GPU work."""
    if not isinstance(settings, dict):
        raise ValueError("the ortho settings must be a dict (got %r)" % (settings,))
    path = settings.get("path")
    if not path or not str(path).endswith(".tif"):
        raise ValueError("the ortho path must end in .tif (got %r)" % (path,))
    if settings.get("border") is None:
        raise ValueError("the ortho settings need a border Xmin,Xmax,Ymin,Ymax[,Zmin,Zmax]")
    z_down = settings.get("z_down", False)
    if z_down not in (False, True, 0, 1):
        raise ValueError("ortho z_down must be a bool (got %r)" % (z_down,))
    from .ortho import TIFF_LIMIT, tiff_layout

    grid = DsmGrid(settings["border"], settings.get("unit") or DEFAULT_UNIT, settings.get("size"))
    if tiff_layout(grid.width, grid.height)[2] >= TIFF_LIMIT:
        raise ValueError("a %d x %d RGBA raster is above the 4 GiB of classic TIFF" % (grid.width, grid.height))
    return grid, bool(z_down)


def add_arguments(ap, prefix=""):
    """The raster of the orthophoto as flags (--<prefix>border, ...); used by this module's CLI and by predict
    (--texture_ortho_*)."""
    ap.add_argument("--%sborder" % prefix, type=parse_border, default=None, help="Xmin,Xmax,Ymin,Ymax[,Zmin,Zmax] (world units)")
    ap.add_argument("--%sunit" % prefix, type=parse_unit, default=None, help="cell size ux,uy (default 0.1,0.1)")
    ap.add_argument("--%ssize" % prefix, type=parse_size, default=None, help="W,H (default from the border and unit, as the DSM)")
    ap.add_argument("--%sz_down" % prefix, action="store_true",
                    help="the lowest surface wins instead of the highest: for scenes whose cameras are on the low-Z side")


def settings_from_args(a, path, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    return {"path": path, "border": g("border"), "unit": g("unit") or list(DEFAULT_UNIT), "size": g("size"), "z_down": bool(g("z_down"))}


def build_and_write(vertices, faces, texcoord, texnumber, atlas, page_row, settings):
    """mesh_to_ortho with the settings dict on device tensors, written with ortho.write_ortho to settings["path"]:
    (rgba, height, summary)."""
    from .ortho import write_ortho

    grid, z_down = check_settings(settings)
    rgba, height = mesh_to_ortho(vertices, faces, texcoord, texnumber, atlas, page_row, grid, z_down)
    write_ortho(settings["path"], rgba, grid)
    return rgba, height, summary(rgba, height)


def read_pages(ply_path, files):
    """The PNG pages a textured PLY names (beside it) as host RGB8 arrays."""
    from PIL import Image

    folder = os.path.dirname(os.path.abspath(str(ply_path)))
    return [np.ascontiguousarray(np.asarray(Image.open(os.path.join(folder, f)).convert("RGB"), np.uint8)) for f in files]


def main(argv=None):
    ap = argparse.ArgumentParser(description="orthophoto of a textured mesh (the PLY and PNG pages texture.write_textured_ply wrote)")
    ap.add_argument("--textured", required=True, help="the textured mesh (.ply; its <stem>_<k>.png pages lie beside it)")
    ap.add_argument("--out", required=True, help="orthophoto file (.tif; the .tfw is written beside it)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.border is None:
        ap.error("--border is required")
    settings = settings_from_args(a, a.out)
    try:
        check_settings(settings)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the orthophoto of the mesh is built on the GPU (no CPU fallback)")
    from .texture import read_textured_ply

    v, f, tc, tn, files = read_textured_ply(a.textured)
    if not files:
        raise ValueError("%s names no texture page" % a.textured)
    pages = read_pages(a.textured, files)
    if len({p.shape[1] for p in pages}) != 1:
        raise ValueError("the pages of %s differ in width" % a.textured)
    atlas, page_row = atlas_from_pages(pages, pages[0].shape[1], "cuda")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rgba, _, s = build_and_write(dev(v), dev(f), dev(tc), dev(tn), atlas, page_row, settings)
    print("orthophoto %s: %d x %d, %d faces, %d pages, %d cells coloured, %d covered but untextured, %d empty"
          % (a.out, rgba.shape[1], rgba.shape[0], f.shape[0], len(pages), s["coloured"], s["untextured"], s["empty"]))
    return a.out


if __name__ == "__main__":
    main()
