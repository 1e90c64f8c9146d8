"""True orthophoto on the DSM.

The reference has no orthophoto step (it stops at the DSM), so the semantics are this project's:

* Grid.  The DSM's DsmGrid: the same size, row 0 north, the same .tfw.  Cell (i, j) is the point
  X = (Xmin + (j + 0.5) ux, Ymax - (i + 0.5) uy, h), h the DSM height as fp64.  A NaN (or infinite) cell is empty.
* Views.  A view has a non-negative integer id (below 2^31 - 1), K [3,3] and E = Tcw [4,4] (the fp32 `outcam` the pipeline
  carries), a depth map [H,W] fp32 and an 8-bit image [H,W,3] of the same size (grey is replicated, an alpha channel
  dropped).  The id is the image id an item carries in outlocation[2], which predict also writes to {name}.txt.
* Projection.  In fp64 with no contraction: p = R X + t, q = K p, each row summed left to right; u = q0 / q2, v = q1 / q2.
  The view is a candidate for the cell when p2 > 0 and q2 > 0, 0 <= u <= W-1 and 0 <= v <= H-1, the depth D at pixel
  (floor(v + 0.5), floor(u + 0.5)) is finite and > 0, and p2 <= D (1 + depth_tolerance): the cell is not behind the surface
  the view saw (default tolerance 0.01, the fusion's default depth threshold).
* Choice.  The score s = (dx^2 + dy^2) / dz^2 in fp64, (dx, dy, dz) = X - C, C = -R^T t: the squared tangent of the angle
  between the ray and the world Z axis, with no sign assumed (Z may point up or down).  A non-finite s rejects the view.  The
  cell's key is (bits(fp32(s)) << 32) | id as a signed int64; the smallest key wins -- the most nadir visible view, ties to the
  lower id.  The empty key is INT64_MAX.  A minimum does not depend on the order in which views are offered, on how they are
  batched, or on which ranks hold them.
* Colour.  Bilinear on the winner's image at (u, v): x0 = floor(u), fx = u - x0 (y alike), taps clamped to the image, the
  weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy summed in that order in fp64, each channel floor(c + 0.5) clamped to
  0..255, alpha 255.  Empty cells and cells no view sees are (0, 0, 0, 0).
* Files.  <name>.tif: little-endian classic TIFF, 8-bit RGBA (4 samples, PhotometricInterpretation RGB, ExtraSamples =
  unassociated alpha), the DSM file's pixel-scale, tie-point and GeoKeyDirectory tags, no GDAL_NODATA.  <name>.tfw:
  grid.tfw_text().  Files above 4 GiB are refused.

The selection and the colouring are HIP kernels (csrc/ortho.hip); there are no atomics, so the rasters are bit-identical for any
batching, order or split of the views.

    python -m deep3d_aerial_amd.ortho --dsm DSM.tif --mvs MVS_FOLDER --out ORTHO.tif [--depth_tolerance 0.01]
        [--image_root DIR] [--views_per_batch N]
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _geom, _lib
from ._geom import batches as _batches, camera_center, check_views_per_batch, ptr as _ptr, stream as _stream
from .dsm import TIFF_LIMIT, DsmGrid, _LONG, _SHORT, assemble_tiff, geo_tags

EMPTY_KEY = (1 << 63) - 1
MAX_ID = (1 << 31) - 2   # id + 1 must fit an int32 (the pipeline's exchange of the winners)
DEFAULT_TOLERANCE = 0.01


_ViewRecord = _lib.STRUCTS["d3d_ortho_view_t"]   # d3d_ortho_view_t, as include/deep3d_planesweep.h declares it


def rgba_image(image):
    """An 8-bit device image [H,W], [H,W,1], [H,W,3] or [H,W,4] -> [H,W,4] uint8 with alpha 255 (grey replicated, alpha
    dropped)."""
    if not isinstance(image, torch.Tensor):
        raise TypeError("image must be a torch.Tensor")
    if not image.is_cuda:
        raise RuntimeError("image is on %s: the orthophoto is built on the GPU (no CPU fallback)" % image.device)
    if image.dtype != torch.uint8:
        raise TypeError("image must be uint8 (got %s)" % image.dtype)
    if image.dim() == 2:
        image = image[:, :, None]
    if image.dim() != 3 or image.shape[2] not in (1, 3, 4):
        raise ValueError("image must be [H,W], [H,W,1], [H,W,3] or [H,W,4] (got %s)" % (tuple(image.shape),))
    rgb = image[:, :, :1].expand(-1, -1, 3) if image.shape[2] == 1 else image[:, :, :3]
    alpha = torch.full(rgb.shape[:2] + (1,), 255, dtype=torch.uint8, device=image.device)
    return torch.cat([rgb, alpha], 2).contiguous()


class OrthoView(_geom.IdCamera):
    """One view offered to the orthophoto: id, K [3,3], E = Tcw [4,4] (host arrays, used in fp64), depth [H,W] fp32 and image
    [H,W(,C)] uint8 on the GPU.  The RGBA8 copy the kernels read is made here."""

    def __init__(self, id, K, E, depth, image):
        from .ops import _chk

        if int(id) != id or not 0 <= int(id) <= MAX_ID:
            raise ValueError("view id %r must be an integer in 0..%d" % (id, MAX_ID))
        _geom.IdCamera.__init__(self, id, K, E)
        _chk(depth, "depth", 2)
        self.depth = depth
        self.rgba = rgba_image(image)
        if tuple(self.rgba.shape[:2]) != tuple(depth.shape):
            raise ValueError("view %d: image %dx%d and depth map %dx%d differ in size" % (self.id, self.rgba.shape[1], self.rgba.shape[0],
                                                                                        depth.shape[1], depth.shape[0]))
        if self.rgba.device != depth.device:
            raise ValueError("view %d: image and depth map on different devices" % self.id)
        self.H, self.W = (int(s) for s in depth.shape)

    def record(self):
        r = self.fill(_ViewRecord())
        r.depth, r.rgba = self.depth.data_ptr(), self.rgba.data_ptr()
        return r


def _records(views, device):
    """The views' d3d_ortho_view_t records in device memory."""
    return _geom.records((_ViewRecord * len(views))(*[v.record() for v in views]), device)


def _check_views(views):
    views = list(views)
    if not all(isinstance(v, OrthoView) for v in views):
        raise TypeError("views must be OrthoView records")
    ids = [v.id for v in views]
    if len(set(ids)) != len(ids):
        raise ValueError("view ids must be unique (got %s)" % sorted(ids))
    return views


def _check_height(height, grid):
    from .ops import _chk

    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    _chk(height, "height", 2)
    if tuple(height.shape) != grid.shape:
        raise ValueError("height %s does not match the grid %d x %d" % (tuple(height.shape), grid.height, grid.width))


def _check_raster(t, name, dtype, shape, device):
    _geom.check_tensor(t, name, dtype, shape, device, "the height")


def check_tolerance(depth_tolerance):
    tol = float(depth_tolerance)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("depth_tolerance %r must be finite and >= 0" % (depth_tolerance,))
    return tol


def select_views(height, grid, views, depth_tolerance=DEFAULT_TOLERANCE, key=None, views_per_batch=None):
    """Min-merges the keys of `views` (OrthoView) into key [H,W] int64 (a new INT64_MAX raster when None) and returns it.
    height: the DSM [H,W] fp32 on the GPU (NaN = empty); views_per_batch: views per d3d_ortho_select call (None: all in one).
    The result does not depend on the batching or the order of the views."""
    _check_height(height, grid)
    tol = check_tolerance(depth_tolerance)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    H, W = grid.shape
    if key is None:
        key = torch.full((H, W), EMPTY_KEY, dtype=torch.int64, device=height.device)
    _check_raster(key, "key", torch.int64, (H, W), height.device)
    lib = _lib.load()
    for batch in _batches(views, vpb):
        recs = _records(batch, height.device)
        scratch, nbytes = _geom.scratch(lib.d3d_ortho_scratch_bytes, W, H, len(batch), device=height.device)
        rc = lib.d3d_ortho_select(_ptr(height), grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], W, H, _ptr(recs), len(batch), tol,
                                  _ptr(scratch), nbytes, _ptr(key), _stream())
        _lib.check(rc, "d3d_ortho_select")
    return key


def colorize(key, height, grid, views, rgba=None, view=None, views_per_batch=None):
    """Colours the cells whose winning id (key's low 32 bits) belongs to one of `views`: rgba [H,W,4] uint8 and view [H,W]
    int32 (new zero / -1 rasters when None) get the bilinear sample and the id; every other cell is left as it is.  height and
    grid must be the ones the keys were selected on.  Returns (rgba, view)."""
    _check_height(height, grid)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    H, W = grid.shape
    _check_raster(key, "key", torch.int64, (H, W), height.device)
    if rgba is None:
        rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device=height.device)
    if view is None:
        view = torch.full((H, W), -1, dtype=torch.int32, device=height.device)
    _check_raster(rgba, "rgba", torch.uint8, (H, W, 4), height.device)
    _check_raster(view, "view", torch.int32, (H, W), height.device)
    lib = _lib.load()
    for batch in _batches(views, vpb):
        recs = _records(batch, height.device)
        rc = lib.d3d_ortho_colorize(_ptr(height), grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], W, H, _ptr(key), _ptr(recs),
                                    len(batch), _ptr(rgba), _ptr(view), _stream())
        _lib.check(rc, "d3d_ortho_colorize")
    return rgba, view


def dsm_to_ortho(height, grid, views, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None):
    """The orthophoto of `views` on the DSM `height`: (rgba [H,W,4] uint8, view [H,W] int32 with -1 for empty, key [H,W]
    int64), queued on the caller's stream."""
    key = select_views(height, grid, views, depth_tolerance, views_per_batch=views_per_batch)
    rgba, view = colorize(key, height, grid, views, views_per_batch=views_per_batch)
    return rgba, view, key


# ----------------------------------------------------------------------------------------
# files: <name>.tif (GeoTIFF, RGBA8) + <name>.tfw
# ----------------------------------------------------------------------------------------
def tiff_layout(width, height):
    """(rows per strip, number of strips, bytes of the file): no allocation."""
    rps = max(1, min(height, (1 << 20) // (4 * width)))
    n_strips = (height + rps - 1) // rps
    return rps, n_strips, 4096 + 8 * n_strips + 4 * width * height


def tiff_bytes(rgba, grid):
    """The .tif file as bytes ([H,W,4] uint8 host array)."""
    H, W = grid.shape
    data = np.ascontiguousarray(rgba, dtype=np.uint8)
    if data.shape != (H, W, 4):
        raise ValueError("rgba %s does not match the grid %d x %d x 4" % (data.shape, H, W))
    rps, n_strips, _ = tiff_layout(W, H)
    counts = [4 * W * min(rps, H - k * rps) for k in range(n_strips)]
    tags = [(256, _LONG, [W]), (257, _LONG, [H]), (258, _SHORT, [8, 8, 8, 8]), (259, _SHORT, [1]), (262, _SHORT, [2]),
            (273, _LONG, [0] * n_strips), (277, _SHORT, [4]), (278, _LONG, [rps]), (279, _LONG, counts), (284, _SHORT, [1]),
            (338, _SHORT, [2]),            # ExtraSamples: unassociated alpha
            (339, _SHORT, [1, 1, 1, 1])] + geo_tags(grid)
    return assemble_tiff(tags, counts, data.tobytes())


def write_ortho(path, rgba, grid):
    """Writes <path> (.tif, RGBA8 GeoTIFF) and the .tfw beside it.  rgba: [H,W,4] uint8 tensor (any device) or array.
    Returns (tif path, tfw path).  Rasters whose file would pass 4 GiB are refused before anything is written."""
    if not isinstance(grid, DsmGrid):
        raise TypeError("grid must be a DsmGrid")
    _, _, total = tiff_layout(grid.width, grid.height)
    if total >= TIFF_LIMIT:
        raise ValueError("a %d x %d RGBA raster needs a %.2f GiB TIFF: above the 4 GiB of classic TIFF (BigTIFF is not "
                         "supported)" % (grid.width, grid.height, total / float(1 << 30)))
    if not str(path).endswith(".tif"):
        raise ValueError("the orthophoto path must end in .tif (got %s)" % path)
    if isinstance(rgba, torch.Tensor):
        rgba = rgba.detach().cpu().numpy()
    blob = tiff_bytes(rgba, grid)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(blob)
    tfw = str(path)[:-4] + ".tfw"
    with open(tfw, "w") as f:
        f.write(grid.tfw_text())
    return str(path), tfw


# ----------------------------------------------------------------------------------------
# predict's products -> views
# ----------------------------------------------------------------------------------------
def center_crop(image, H, W, what="image"):
    """The centre crop of an [h,w(,C)] image to the depth map's H x W, as dataset.crop_window / slice_window choose it at
    resize_scale 1 (start = ceil((h - H) / 2)).  An image smaller than the map is refused."""
    h, w = image.shape[:2]
    if h < H or w < W:
        raise ValueError("%s is %dx%d, smaller than its %dx%d depth map" % (what, w, h, W, H))
    y0, x0 = int(math.ceil((h - H) / 2)), int(math.ceil((w - W) / 2))
    return image[y0:y0 + H, x0:x0 + W]


def load_mvs_views(mvs_folder, image_root=None, device="cuda"):
    """OrthoView records of every {name}_init.pfm + {name}.txt predict wrote under mvs_folder: the camera and the id from the
    camera file (predict.read_red_cam), the image it names (relative paths under image_root, else beside the camera file)
    centre-cropped to the depth map."""
    from . import dataset

    views = []
    for name, cam, location, path in _geom.mvs_cameras(mvs_folder):
        depth = _geom.load_map(mvs_folder, name, "_init", device)
        if not os.path.isabs(path):
            path = os.path.join(image_root if image_root is not None else mvs_folder, path)
        H, W = depth.shape
        crop = np.ascontiguousarray(center_crop(dataset.read_image_u8(path), H, W, path))
        views.append(OrthoView(int(location[2]), cam[1, :3, :3], cam[0], depth, torch.from_numpy(crop).to(device)))
    return views


def add_arguments(ap, prefix=""):
    ap.add_argument("--%sdepth_tolerance" % prefix, type=float, default=DEFAULT_TOLERANCE,
                    help="a cell is hidden from a view when its depth exceeds the view's depth map by more than this share")
    ap.add_argument("--%sviews_per_batch" % prefix, type=int, default=None, help="views per selection call (default: all)")


def check_args(ap, a, prefix=""):
    """The argument errors of the ortho settings, reported through ap.error."""
    tol = getattr(a, prefix + "depth_tolerance")
    if not (math.isfinite(tol) and tol >= 0.0):
        ap.error("--%sdepth_tolerance %g must be finite and >= 0" % (prefix, tol))
    vpb = getattr(a, prefix + "views_per_batch")
    if vpb is not None and vpb < 1:
        ap.error("--%sviews_per_batch must be >= 1" % prefix)


def settings_from_args(a, path, prefix=""):
    return {"path": path, "depth_tolerance": getattr(a, prefix + "depth_tolerance"),
            "views_per_batch": getattr(a, prefix + "views_per_batch")}


def main(argv=None):
    ap = argparse.ArgumentParser(description="true orthophoto from a DSM and predict's depth maps, cameras and images")
    ap.add_argument("--dsm", required=True, help="the DSM (.tif) dsm.write_dsm wrote")
    ap.add_argument("--mvs", required=True, help="predict's output folder: {name}_init.pfm and {name}.txt")
    ap.add_argument("--out", required=True, help="orthophoto file (.tif; the .tfw is written beside it)")
    ap.add_argument("--image_root", default=None, help="folder the camera files' relative image paths start from")
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_args(ap, a)
    if not torch.cuda.is_available():
        raise RuntimeError("the orthophoto is built on the GPU (no CPU fallback)")
    from .dsm import read_dsm

    h, grid = read_dsm(a.dsm)
    height = torch.from_numpy(h).cuda()
    views = load_mvs_views(a.mvs, a.image_root)
    rgba, view, _ = dsm_to_ortho(height, grid, views, a.depth_tolerance, a.views_per_batch)
    write_ortho(a.out, rgba, grid)
    print("orthophoto %s: %d x %d, %d views, %d cells coloured" % (a.out, grid.width, grid.height, len(views),
                                                                  int((view >= 0).sum())))
    return a.out


if __name__ == "__main__":
    main()
