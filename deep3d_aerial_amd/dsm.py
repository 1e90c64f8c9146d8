"""Digital surface model (DSM) from the fused point cloud.

The reference's CREATEDSM step with dsm_source "pc" (config.yaml; run.py:209-247) calls pc2dsm.DSM_from_PC, which the
reference never shipped (dsm/readme.txt is a download link), so the semantics here are this project's, following the
reference wherever it says anything:

* Grid.  border = [Xmin, Xmax, Ymin, Ymax(, Zmin, Zmax)] and unit = (ux, uy) in world units, Z the height.  The raster is the
  explicit size (W, H) if given, else W = int((Xmax - Xmin + 1e-8) / ux), H = int((Ymax - Ymin + 1e-8) / uy) -- what the
  reference's gdal_create_dsm_file creates (IO/gdal_io.py:122-134).  Row 0 is north: a point's cell is
  j = floor((x - Xmin) / ux), i = floor((Ymax - y) / uy), in fp64.  A point is kept when x, y, z are finite, the cell lies in
  the raster and Zmin <= z <= Zmax (when the border has Z bounds).
* Order.  Heights are compared in the IEEE total order (-0.0 < +0.0): every selection is exact and independent of the order
  of the points.
* Selection.  "Max": the largest z of the cell.  "Robust_Max" (this project's definition): with the cell's n heights sorted
  in descending order, drop the top t = floor(trim * n) and take the (t+1)-th largest; with trim 0.1 a cell of fewer than
  10 points gets its plain maximum.  Under either method a cell of fewer than min_points points is empty (NaN).
* Interpolation.  None by default.  "MovingAverage" fills only empty cells, each with the mean of the non-empty cells of the
  (2 radius + 1)^2 window around it (clipped to the raster; summed in fp64 in a fixed order, rounded once), radius 1..16;
  a cell with no non-empty neighbour stays empty; `iterations` passes, each reading the previous one's output.
* Files.  <name>.tif: little-endian classic TIFF, one float32 band, GeoTIFF pixel scale / tie point, a GeoKeyDirectory with
  PixelIsArea and no CRS (the reference has none), GDAL_NODATA; empty cells written as `nodata`.  <name>.tfw: the text
  gdal_create_dsm_file writes.  Rasters whose file would pass 4 GiB are refused (BigTIFF is out of scope).

The binning, the per-cell selection and the fill are HIP kernels (csrc/dsm.hip); the results are bit-reproducible for any
order or split of the points.

DSM from a triangle mesh: the reference's default dsm_source "mesh" (run.py:226-232 calls
mesh2dsm.DSM_from_Mesh, also never shipped).  mesh_to_dsm rasterises vertices [n,3] fp32 and faces [m,3] int32 on the same
grid, origin, row order and files:

* Samples.  Cell (i, j) samples its centre cx = Xmin + (j + .5) ux, cy = Ymax - (i + .5) uy, in fp64.
* Triangles.  A face (a, b, c) is used when its indices are in range (mesh_to_dsm refuses others with a ValueError before any
  launch) and its nine coordinates are finite; its vertices are first put in lexicographic (x, y, z) order (IEEE total order
  per component), so nothing below depends on the winding or on which vertex comes first.  Everything is fp64 with no
  contraction.  For a directed edge p -> q with endpoints (u, v) in lexicographic (x, y) order and s = +1 if (u, v) == (p, q),
  else -1: E(p, q, P) = s ((v.x - u.x)(P.y - u.y) - (v.y - u.y)(P.x - u.x)).  Two triangles that share an edge evaluate the
  same magnitudes on it, so with the inclusive rule below the raster has no cracks along shared edges.
* Coverage.  D = E(a, b, c); a triangle whose D is 0 or not finite (vertical walls, degenerate triangles) contributes nothing.
  Else sigma = sign(D), w_a = sigma E(b, c, P), w_b = sigma E(c, a, P), w_c = sigma E(a, b, P); the centre is covered when
  all three are >= 0 and W = (w_a + w_b) + w_c > 0, and the sample is z = ((w_a z_a + w_b z_b) + w_c z_c) / W rounded once to
  fp32.  Only the centres of the triangle's cell range are tested: columns floor((x_lo - Xmin) / ux) - 1 ..
  floor((x_hi - Xmin) / ux) + 1 and rows floor((Ymax - y_hi) / uy) - 1 .. floor((Ymax - y_lo) / uy) + 1 of its XY box,
  clipped to the raster (a one-cell margin around every centre the box holds).
* Selection.  A sample outside [Zmin, Zmax] (when the border has Z bounds) is dropped; a cell's height is its largest sample
  in the IEEE total order, NaN when it has none.  Only "Max" exists for this source (min_points is 1).  The optional
  MovingAverage fill is the one above, applied after the raster.
* The raster is a function of the set of triangles: not of their order, their winding or how the list is split.

    python -m deep3d_aerial_amd.dsm (--fused DIR | --mesh FILE.ply) --out FILE.tif --border Xmin,Xmax,Ymin,Ymax[,Zmin,Zmax]
        --unit ux,uy [--size W,H] [--select Max|Robust_Max] [--trim 0.1] [--min_points 1]
        [--interpolation none|MovingAverage] [--radius 2] [--iterations 1] [--nodata -9999]
"""
import argparse
import math
import os
import struct

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream

SELECT = {"Max": 0, "Robust_Max": 1}
INTERPOLATION = (None, "none", "MovingAverage")
MAX_RADIUS = 16
DSM_TRI_SMALL = 64     # csrc/dsm.hip: triangles whose cell range holds at most this many cells take one lane and no list
SOURCES = ("pc", "mesh")
TIFF_LIMIT = 1 << 32   # classic TIFF: 32-bit offsets


class DsmGrid(object):
    """The raster of a DSM: border [Xmin, Xmax, Ymin, Ymax(, Zmin, Zmax)], unit (ux, uy), size (W, H) or None."""

    def __init__(self, border, unit, size=None):
        border = [float(b) for b in border]
        if len(border) not in (4, 6):
            raise ValueError("border must be [Xmin, Xmax, Ymin, Ymax] or [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax] (got %d values)"
                             % len(border))
        unit = [float(u) for u in (unit if np.ndim(unit) else (unit, unit))]
        if len(unit) != 2:
            raise ValueError("unit must be (ux, uy)")
        self.border, self.unit = border, tuple(unit)
        self.x_min, self.x_max, self.y_min, self.y_max = border[:4]
        self.z_min, self.z_max = (border[4], border[5]) if len(border) == 6 else (-math.inf, math.inf)
        if not all(math.isfinite(u) and u > 0 for u in unit):
            raise ValueError("unit (%g, %g) must be finite and > 0" % tuple(unit))
        if size is None:   # gdal_create_dsm_file (IO/gdal_io.py:123-124)
            self.width = int((self.x_max - self.x_min + 0.00000001) / unit[0])
            self.height = int((self.y_max - self.y_min + 0.00000001) / unit[1])
        else:
            if len(size) != 2:
                raise ValueError("size must be (W, H)")
            self.width, self.height = int(size[0]), int(size[1])
        if self.width < 1 or self.height < 1:
            raise ValueError("empty raster %d x %d" % (self.width, self.height))
        if self.width * self.height >= 1 << 31:
            raise ValueError("raster %d x %d: W * H must stay below 2^31" % (self.width, self.height))

    @property
    def shape(self):
        return (self.height, self.width)

    def tfw_text(self):
        """The world file gdal_create_dsm_file writes (IO/gdal_io.py:129-130), byte for byte."""
        ux, uy = self.unit
        return str(ux) + "\n0\n0\n" + str(-uy) + "\n" + str(self.border[0]) + "\n" + str(self.border[3])

    def _raster(self):
        return (self.x_min, self.y_max, self.unit, self.width, self.height)

    def __eq__(self, other):
        """Equal rasters: the same origin (Xmin, Ymax), unit and size -- every cell and the .tfw agree.  The Z bounds only
        filter points and are not compared."""
        return isinstance(other, DsmGrid) and self._raster() == other._raster()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._raster())

    def __repr__(self):
        return "DsmGrid(border=%s, unit=%s, size=(%d, %d))" % (self.border, self.unit, self.width, self.height)


def check_grid(raster, grid, name):
    """grid is a DsmGrid, and an [H,W] tensor `raster` (`name` in the message) has its shape."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    if isinstance(raster, torch.Tensor) and raster.dim() == 2 and tuple(raster.shape) != grid.shape:
        raise ValueError("%s %s does not match the grid %d x %d" % (name, tuple(raster.shape), grid.height, grid.width))


def fill_moving_average(height, radius=2, iterations=1):
    """MovingAverage hole fill of an [H,W] fp32 device raster (NaN = empty): `iterations` launches of
    d3d_dsm_fill_moving_average, ping-ponging two rasters.  Returns a new tensor; the input is not changed."""
    from .ops import _chk

    _chk(height, "height", 2)
    if not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("radius %d outside 1..%d" % (radius, MAX_RADIUS))
    if int(iterations) < 1:
        raise ValueError("iterations must be >= 1")
    H, W = (int(s) for s in height.shape)
    lib = _lib.load()
    src, bufs = height, [torch.empty_like(height), torch.empty_like(height)]
    for k in range(int(iterations)):
        dst = bufs[k % 2]
        _lib.check(lib.d3d_dsm_fill_moving_average(_ptr(src), _ptr(dst), W, H, int(radius), _stream()),
                   "d3d_dsm_fill_moving_average")
        src = dst
    return src


def points_to_dsm(xyz, grid, select="Max", trim=0.1, min_points=1, interpolation=None, radius=2, iterations=1):
    """xyz [N,3] fp32 device points -> (height [H,W] fp32 with NaN for empty cells, count [H,W] int32 kept points per cell),
    queued on the caller's stream.  select "Max" | "Robust_Max", trim in [0, 1) (Robust_Max), min_points >= 1,
    interpolation None | "none" | "MovingAverage" (radius 1..16, iterations >= 1).  CPU tensors are refused."""
    from .ops import _chk

    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    if select not in SELECT:
        raise ValueError("select %r: one of %s" % (select, ", ".join(SELECT)))
    fill = _check_fill(interpolation, radius, iterations)
    p = _chk(xyz, "xyz", 2)
    if xyz.shape[1] != 3:
        raise ValueError("xyz must be [N,3] (got %s)" % (tuple(xyz.shape),))
    n = int(xyz.shape[0])
    H, W = grid.shape
    lib = _lib.load()
    mode = SELECT[select]
    height = torch.empty((H, W), dtype=torch.float32, device=xyz.device)
    count = torch.empty((H, W), dtype=torch.int32, device=xyz.device)
    scratch, nbytes = _geom.scratch(lib.d3d_dsm_scratch_bytes, n, W, H, mode, device=xyz.device)
    if nbytes == 0 and n >= 1 << 31:
        raise ValueError("%d points: at most 2^31 - 1" % n)
    rc = lib.d3d_dsm_from_points(p if n else None, n, grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], grid.z_min, grid.z_max,
                                 W, H, mode, float(trim), int(min_points), _ptr(scratch), nbytes, _ptr(height), _ptr(count), _stream())
    _lib.check(rc, "d3d_dsm_from_points")
    if fill:
        height = fill_moving_average(height, radius, iterations)
    return height, count


def _check_fill(interpolation, radius, iterations):
    if interpolation not in INTERPOLATION:
        raise ValueError("interpolation %r: None, 'none' or 'MovingAverage'" % (interpolation,))
    fill = interpolation == "MovingAverage"
    if fill and not 1 <= int(radius) <= MAX_RADIUS:   # before any launch
        raise ValueError("radius %d outside 1..%d" % (radius, MAX_RADIUS))
    if fill and int(iterations) < 1:
        raise ValueError("iterations must be >= 1")
    return fill


def mesh_to_dsm(vertices, faces, grid, interpolation=None, radius=2, iterations=1):
    """vertices [n,3] fp32 and faces [m,3] int32 device tensors -> height [H,W] fp32 with NaN for empty cells (the mesh
    semantics of this module's docstring), queued on the caller's stream.  interpolation None | "none" | "MovingAverage"
    (radius 1..16, iterations >= 1).  CPU tensors are refused; so are face indices outside 0..n-1 (ValueError, before any
    launch: this check reads the index range back to the host)."""
    from .ops import _chk

    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    fill = _check_fill(interpolation, radius, iterations)
    if not isinstance(vertices, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise TypeError("vertices and faces must be torch.Tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be [n,3] (got %s)" % (tuple(vertices.shape),))
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise ValueError("faces must be a contiguous [m,3] int32 tensor (got %s %s)" % (faces.dtype, tuple(faces.shape)))
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if nv >= 1 << 31 or nf >= 1 << 31:
        raise ValueError("%d vertices, %d faces: at most 2^31 - 1 of each" % (nv, nf))
    if nf:
        lo, hi = torch.stack([faces.min(), faces.max()]).tolist()
        if lo < 0 or hi >= nv:
            raise ValueError("face indices span %d..%d: outside the %d vertices" % (lo, hi, nv))
    pv = _chk(vertices, "vertices", 2)
    if not faces.is_cuda:
        raise RuntimeError("faces is on %s: the DSM is built on the GPU (no CPU fallback)" % faces.device)
    if faces.device != vertices.device:
        raise ValueError("vertices on %s, faces on %s" % (vertices.device, faces.device))
    H, W = grid.shape
    lib = _lib.load()
    height = torch.empty((H, W), dtype=torch.float32, device=vertices.device)
    scratch, nbytes = _geom.scratch(lib.d3d_dsm_mesh_scratch_bytes, nf, W, H, device=vertices.device)
    rc = lib.d3d_dsm_from_mesh(pv if nv else None, nv, _ptr(faces) if nf else None, nf, grid.x_min, grid.y_max, grid.unit[0],
                               grid.unit[1], grid.z_min, grid.z_max, W, H, _ptr(scratch), nbytes, _ptr(height), _stream())
    _lib.check(rc, "d3d_dsm_from_mesh")
    if fill:
        height = fill_moving_average(height, radius, iterations)
    return height


# ----------------------------------------------------------------------------------------
# files: <name>.tif (GeoTIFF, float32) + <name>.tfw
# ----------------------------------------------------------------------------------------
_SHORT, _ASCII, _LONG, _DOUBLE = 3, 2, 4, 12
_TYPE_SIZE = {_SHORT: 2, _ASCII: 1, _LONG: 4, _DOUBLE: 8}
_TYPE_FMT = {_SHORT: "H", _LONG: "I", _DOUBLE: "d"}


def _nodata_text(v):
    v = float(v)
    return ("%d" % v) if v.is_integer() else repr(v)


def tiff_layout(width, height):
    """(rows per strip, number of strips, bytes of the header + IFD + tag data + pixels): no allocation."""
    rps = max(1, min(height, (1 << 20) // (4 * width)))
    n_strips = (height + rps - 1) // rps
    meta = 4096 + 8 * n_strips   # header, IFD and tag data: a bound
    return rps, n_strips, meta + 4 * width * height


def tiff_bytes(height_map, grid, nodata=-9999.0):
    """The .tif file as bytes ([H,W] float32 host array, NaN = empty)."""
    H, W = grid.shape
    rps, n_strips, _ = tiff_layout(W, H)
    data = np.ascontiguousarray(height_map, dtype="<f4")
    if data.shape != (H, W):
        raise ValueError("height map %s does not match the grid %d x %d" % (data.shape, H, W))
    data = np.where(np.isnan(data), np.float32(nodata), data).astype("<f4")
    nodata_txt = _nodata_text(nodata).encode("ascii") + b"\0"
    row_bytes = 4 * W
    counts = [row_bytes * min(rps, H - k * rps) for k in range(n_strips)]
    tags = [(256, _LONG, [W]), (257, _LONG, [H]), (258, _SHORT, [32]), (259, _SHORT, [1]), (262, _SHORT, [1]),
            (273, _LONG, [0] * n_strips), (277, _SHORT, [1]), (278, _LONG, [rps]), (279, _LONG, counts), (284, _SHORT, [1]),
            (339, _SHORT, [3])] + geo_tags(grid) + [(42113, _ASCII, nodata_txt)]                # GDAL_NODATA
    return assemble_tiff(tags, counts, data.tobytes())


def geo_tags(grid):
    """The GeoTIFF tags of a raster on `grid`: pixel scale, tie point and a GeoKeyDirectory with PixelIsArea and no CRS."""
    # GeoKeyDirectory: version 1.1.0, one key: GTRasterTypeGeoKey (1025) = RasterPixelIsArea (1); no CRS keys
    geokeys = [1, 1, 0, 1, 1025, 0, 1, 1]
    return [(33550, _DOUBLE, [grid.unit[0], grid.unit[1], 0.0]),                       # ModelPixelScaleTag
            (33922, _DOUBLE, [0.0, 0.0, 0.0, grid.border[0], grid.border[3], 0.0]),     # ModelTiepointTag: pixel (0, 0) -> (Xmin, Ymax)
            (34735, _SHORT, geokeys)]                                                   # GeoKeyDirectoryTag


def assemble_tiff(tags, counts, pixels):
    """A little-endian classic TIFF: header, one IFD of `tags` [(tag, type, values)] in ascending tag order (StripOffsets, 273,
    is filled in here), the tag data that does not fit an entry, then the strips of `counts` bytes each (`pixels`)."""
    n_strips = len(counts)
    ifd_at = 8
    extra_at = ifd_at + 2 + 12 * len(tags) + 4
    blobs, entries, at = [], [], extra_at

    def payload(typ, vals):
        return bytes(vals) if typ == _ASCII else struct.pack("<%d%s" % (len(vals), _TYPE_FMT[typ]), *vals)

    # tag data that does not fit the 4-byte field goes behind the IFD; strip offsets are known once that size is
    sizes = [len(v) * _TYPE_SIZE[t] for _, t, v in tags]
    extra = sum((s + 1) & ~1 for s in sizes if s > 4)
    pixels_at = extra_at + extra
    strip_offsets = [pixels_at + sum(counts[:k]) for k in range(n_strips)]
    for tag, typ, vals in tags:
        if tag == 273:
            vals = strip_offsets
        raw = payload(typ, vals)
        if len(raw) <= 4:
            entries.append(struct.pack("<HHI", tag, typ, len(vals)) + raw.ljust(4, b"\0"))
        else:
            entries.append(struct.pack("<HHII", tag, typ, len(vals), at))
            blobs.append(raw + (b"\0" if len(raw) % 2 else b""))
            at += len(blobs[-1])
    assert at == pixels_at
    head = b"II" + struct.pack("<HI", 42, ifd_at) + struct.pack("<H", len(tags)) + b"".join(entries) + struct.pack("<I", 0)
    return head + b"".join(blobs) + pixels


def write_dsm(path, height, grid, nodata=-9999.0):
    """Writes <path> (.tif, float32 GeoTIFF, empty cells as `nodata`) and the .tfw beside it.  height: [H,W] fp32 tensor (any
    device) or array, NaN = empty.  Returns (tif path, tfw path).  Rasters whose file would pass 4 GiB are refused before
    anything is allocated or written."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    _, _, total = tiff_layout(grid.width, grid.height)
    if total >= TIFF_LIMIT:
        raise ValueError("a %d x %d float32 raster needs a %.2f GiB TIFF: above the 4 GiB of classic TIFF (BigTIFF is not "
                         "supported)" % (grid.width, grid.height, total / float(1 << 30)))
    if not str(path).endswith(".tif"):
        raise ValueError("the DSM path must end in .tif (got %s)" % path)
    if isinstance(height, torch.Tensor):
        height = height.detach().cpu().numpy()
    blob = tiff_bytes(height, grid, nodata)
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    with open(path, "wb") as f:
        f.write(blob)
    tfw = str(path)[:-4] + ".tfw"
    with open(tfw, "w") as f:
        f.write(grid.tfw_text())
    return str(path), tfw


def _ifd(blob, what):
    """{tag: values} of the first IFD of a little-endian classic TIFF (the layout tiff_bytes writes), else ValueError."""
    if len(blob) < 8 or blob[:4] != b"II*\0":
        raise ValueError("%s: not a little-endian classic TIFF (BigTIFF and big-endian files are not read)" % what)
    ifd_at = struct.unpack_from("<I", blob, 4)[0]
    if ifd_at + 2 > len(blob):
        raise ValueError("%s: truncated TIFF" % what)
    n = struct.unpack_from("<H", blob, ifd_at)[0]
    if ifd_at + 2 + 12 * n > len(blob):
        raise ValueError("%s: truncated TIFF" % what)
    tags = {}
    for k in range(n):
        tag, typ, count = struct.unpack_from("<HHI", blob, ifd_at + 2 + 12 * k)
        if typ not in _TYPE_SIZE:
            raise ValueError("%s: tag %d has TIFF type %d, which this reader does not take" % (what, tag, typ))
        size = count * _TYPE_SIZE[typ]
        at = ifd_at + 2 + 12 * k + 8 if size <= 4 else struct.unpack_from("<I", blob, ifd_at + 2 + 12 * k + 8)[0]
        if at + size > len(blob):
            raise ValueError("%s: truncated TIFF (tag %d)" % (what, tag))
        tags[tag] = blob[at:at + size] if typ == _ASCII else list(struct.unpack_from("<%d%s" % (count, _TYPE_FMT[typ]), blob, at))
    return tags


def read_dsm(path):
    """A DSM file this project wrote (write_dsm) -> (height [H,W] float32 host array with NaN where the file holds its
    GDAL_NODATA value, DsmGrid).  The grid comes from the size, the pixel scale and the tie point: border
    [Xmin, Xmin + W ux, Ymax - H uy, Ymax], unit (ux, uy), size (W, H).  Any other TIFF layout (compression, tiles, several
    bands, another sample type, no georeferencing) is refused with a ValueError."""
    with open(path, "rb") as f:
        blob = f.read()
    t = _ifd(blob, path)
    want = {258: [32], 259: [1], 277: [1], 339: [3]}
    for tag, v in want.items():
        if t.get(tag, [1] if tag == 277 else None) != v:
            raise ValueError("%s: not a DSM file of this project (tag %d is %s, expected %s: one uncompressed float32 band)"
                             % (path, tag, t.get(tag), v))
    if t.get(284, [1]) != [1] or 322 in t:
        raise ValueError("%s: tiled or planar-separate TIFFs are not read" % path)
    for tag, name in ((256, "ImageWidth"), (257, "ImageLength"), (273, "StripOffsets"), (279, "StripByteCounts"),
                      (33550, "ModelPixelScale"), (33922, "ModelTiepoint")):
        if tag not in t:
            raise ValueError("%s: no %s tag: not a DSM file of this project" % (path, name))
    W, H = int(t[256][0]), int(t[257][0])
    scale, tie = t[33550], t[33922]
    if len(scale) < 2 or len(tie) < 6 or tie[:3] != [0.0, 0.0, 0.0]:
        raise ValueError("%s: the tie point must map pixel (0, 0); got %s" % (path, tie))
    offsets, counts = t[273], t[279]
    if len(offsets) != len(counts) or sum(counts) != 4 * W * H or any(o + c > len(blob) for o, c in zip(offsets, counts)):
        raise ValueError("%s: the strips do not hold %d x %d float32 values" % (path, W, H))
    data = b"".join(blob[o:o + c] for o, c in zip(offsets, counts))
    height = np.frombuffer(data, dtype="<f4").reshape(H, W).astype(np.float32)
    if 42113 in t:
        nodata = np.float32(float(t[42113].rstrip(b"\0").decode("ascii")))
        height = np.where(height == nodata, np.float32(np.nan), height).astype(np.float32)
    ux, uy = float(scale[0]), float(scale[1])
    x_min, y_max = float(tie[3]), float(tie[4])
    grid = DsmGrid([x_min, x_min + W * ux, y_max - H * uy, y_max], [ux, uy], size=(W, H))
    return height, grid


def load_fused_xyz(folder):
    """The xyz [n,3] float32 of every .npz pipeline.save_fused wrote under `folder` (scene sub-folders included), in sorted
    path order and concatenated; duplicates across scene blocks are kept."""
    parts = []
    for root, dirs, files in os.walk(folder):
        dirs.sort()
        for f in sorted(files):
            if f.endswith(".npz"):
                with np.load(os.path.join(root, f)) as d:
                    parts.append(np.asarray(d["xyz"], np.float32).reshape(-1, 3))
    if not parts:
        raise FileNotFoundError("no fused .npz arrays under %s" % folder)
    return np.concatenate(parts, 0)


def _floats(text, n=None, what="value"):
    vals = [float(v) for v in str(text).split(",") if v.strip()]
    if n is not None and len(vals) not in (n if isinstance(n, tuple) else (n,)):
        raise argparse.ArgumentTypeError("%s: expected %s comma-separated numbers" % (what, n))
    return vals


def parse_border(text):
    return _floats(text, (4, 6), "border")


def parse_unit(text):
    v = _floats(text, (1, 2), "unit")
    return v * 2 if len(v) == 1 else v


def parse_size(text):
    return [int(v) for v in _floats(text, 2, "size")]


def build_and_write(xyz, settings, device="cuda"):
    """settings: {"path", "border", "unit", "size", "select", "trim", "min_points", "interpolation", "radius", "iterations",
    "nodata"} (predict --dsm_*, mvs_dl.dsm_settings) -> writes the .tif / .tfw; returns (height, count)."""
    grid = DsmGrid(settings["border"], settings.get("unit") or (0.1, 0.1), settings.get("size"))
    if not isinstance(xyz, torch.Tensor):
        xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float32))
    xyz = xyz.to(device=device, dtype=torch.float32).contiguous()
    h, c = points_to_dsm(xyz, grid, select=settings.get("select", "Max"), trim=settings.get("trim", 0.1),
                         min_points=settings.get("min_points", 1), interpolation=settings.get("interpolation"),
                         radius=settings.get("radius", 2), iterations=settings.get("iterations", 1))
    write_dsm(settings["path"], h, grid, nodata=settings.get("nodata", -9999.0))
    return h, c


def check_mesh_settings(settings):
    """The settings a mesh DSM cannot honour, refused before any work: only "Max" exists and min_points is 1."""
    if settings.get("select", "Max") != "Max":
        raise ValueError("a DSM from the mesh has only select 'Max' (got %r)" % (settings.get("select"),))
    if int(settings.get("min_points", 1)) != 1:
        raise ValueError("a DSM from the mesh has no min_points (got %d; leave it at 1)" % int(settings.get("min_points")))


def build_and_write_mesh(vertices, faces, settings, device="cuda"):
    """The DSM of a mesh (vertices [n,3], faces [m,3]; tensors or arrays) with the settings of build_and_write ("select" Max,
    "min_points" 1; "trim" is ignored) -> writes the .tif / .tfw; returns height."""
    check_mesh_settings(settings)
    grid = DsmGrid(settings["border"], settings.get("unit") or (0.1, 0.1), settings.get("size"))
    to = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=device, dtype=dt).contiguous()
    h = mesh_to_dsm(to(vertices, torch.float32).reshape(-1, 3), to(faces, torch.int32).reshape(-1, 3), grid,
                    interpolation=settings.get("interpolation"), radius=settings.get("radius", 2),
                    iterations=settings.get("iterations", 1))
    write_dsm(settings["path"], h, grid, nodata=settings.get("nodata", -9999.0))
    return h


def add_arguments(ap, prefix=""):
    """The DSM settings as flags (--<prefix>border, ...); used by this module's CLI and by predict (--dsm_*)."""
    ap.add_argument("--%sborder" % prefix, type=parse_border, default=None, help="Xmin,Xmax,Ymin,Ymax[,Zmin,Zmax] (world units)")
    ap.add_argument("--%sunit" % prefix, type=parse_unit, default=[0.1, 0.1], help="cell size ux,uy (run.py:218 default 0.1,0.1)")
    ap.add_argument("--%ssize" % prefix, type=parse_size, default=None, help="W,H (default from the border and unit, as gdal_io)")
    ap.add_argument("--%sselect" % prefix, default="Max", choices=list(SELECT), help="per-cell height (pc_select_method)")
    ap.add_argument("--%strim" % prefix, type=float, default=0.1, help="Robust_Max: share of the highest points dropped per cell")
    ap.add_argument("--%smin_points" % prefix, type=int, default=1, help="cells with fewer points are empty")
    ap.add_argument("--%sinterpolation" % prefix, default="none", choices=["none", "MovingAverage"],
                    help="hole fill (pc_interpolation_method)")
    ap.add_argument("--%sradius" % prefix, type=int, default=2, help="MovingAverage window radius, 1..16")
    ap.add_argument("--%siterations" % prefix, type=int, default=1, help="MovingAverage passes")
    ap.add_argument("--%snodata" % prefix, type=float, default=-9999.0, help="value written for empty cells")


def settings_from_args(a, path, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    interp = g("interpolation")
    return {"path": path, "border": g("border"), "unit": g("unit"), "size": g("size"), "select": g("select"), "trim": g("trim"),
            "min_points": g("min_points"), "interpolation": None if interp in (None, "none") else interp, "radius": g("radius"),
            "iterations": g("iterations"), "nodata": g("nodata")}


def check_mesh_args(ap, a, prefix=""):
    """Argument errors for a DSM from the mesh: the point-only settings away from their defaults."""
    if getattr(a, prefix + "select") != "Max":
        ap.error("a DSM from the mesh has only --%sselect Max" % prefix)
    if getattr(a, prefix + "min_points") != 1:
        ap.error("a DSM from the mesh has no --%smin_points (leave it at 1)" % prefix)


def main(argv=None):
    ap = argparse.ArgumentParser(description="DSM from the fused point cloud (pipeline.save_fused's .npz arrays) or from a mesh")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--fused", help="folder of the fused arrays (scene sub-folders included)")
    src.add_argument("--mesh", help="mesh file (.ply, as mesh.write_ply writes it)")
    ap.add_argument("--out", required=True, help="DSM file (.tif; the .tfw is written beside it)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.border is None:
        ap.error("--border is required")
    if a.mesh is not None:
        check_mesh_args(ap, a)
    if not torch.cuda.is_available():
        raise RuntimeError("the DSM is built on the GPU (no CPU fallback)")
    if a.mesh is not None:
        from . import mesh as _mesh

        v, f = _mesh.read_ply(a.mesh)
        h = build_and_write_mesh(v, f, settings_from_args(a, a.out))
        print("DSM %s: %d x %d, %d triangles, %d cells filled" % (a.out, h.shape[1], h.shape[0], f.shape[0],
                                                                 int(torch.isfinite(h).sum())))
        return a.out
    xyz = load_fused_xyz(a.fused)
    h, c = build_and_write(xyz, settings_from_args(a, a.out))
    print("DSM %s: %d x %d, %d points, %d cells filled" % (a.out, h.shape[1], h.shape[0], xyz.shape[0],
                                                          int(torch.isfinite(h).sum())))
    return a.out


if __name__ == "__main__":
    main()
