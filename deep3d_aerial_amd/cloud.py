"""Voxel-grid merge of the fused points into one de-duplicated point cloud with colour, normal and support count, written as a
binary PLY.

The reference's first product is the dense cloud: Fuse_Depth_Map.batch_fuse_depths writes one coloured .ply with normals per scene
block, run.py copies it to production/Point_Cloud, and reserves a Resample_PC folder that nothing fills.  This stage stands where
Resample_PC would.  The rule below is this project's own; it does not claim to match any tool.

* Grid.  CloudGrid(border, voxel): border = [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax], all six finite with min < max; voxel = v > 0,
  finite; n_a = ceil((max_a - min_a) / v) per axis, each in 1 .. 2^21 - 1, else ValueError.
* Cell of a point.  Per axis u = ((double)x - min_a) / v in fp64, i = floor(u), r = floor((u - i) * 65536), which lies in
  0 .. 65535.  A point is dropped when a coordinate is not finite or an i is outside 0 .. n_a - 1; a point exactly on a max face
  whose u equals n_a is therefore dropped.  Key: (iz << 42) | (iy << 21) | ix, 63 bits; a dropped point gets the key INT64_MAX.
* Per occupied voxel all sums are integer sums over its members, so the grouping and order of the additions cannot change a bit.
  - count: the number of members, int32.
  - Position, per axis: S = sum r; min_a + (i + (S + 0.5 count) / (65536.0 count)) * v in fp64, each operation rounded once (no
    fused multiply-add), then rounded to fp32.  It is within v / 65536 plus one fp32 ulp of the exact mean of the members: each
    r + 0.5 is within half a 65536th of a voxel of its u - i, and the fp64 roundings are far below the fp32 one.
  - Normal, when normals are given: per component llrint(n_c * 2^20) as int64 is summed; a member whose normal has a non-finite
    component adds nothing, and neither does one with a component of magnitude above 1024 (a unit normal is far below it; the bound
    keeps 2^31 members from overflowing int64).  Output sum / |sum| in fp64, |sum| = sqrt((x x + y y) + z z), rounded to fp32;
    (0, 0, 0) when the sum vector is zero.
  - Colour, when colours are given (int32 [n,3], each channel clamped to 0 .. 255 on input): per channel
    (2 sum + count) // (2 count), as uint8: the mean with .5 rounded up.
* Isolated voxels.  min_points = K >= 1; the default 1 means off.  A voxel is kept when the counts of its 3 x 3 x 3 neighbourhood,
  the voxel itself included, sum to at least K.  Neighbours outside the grid do not exist.  The sum is taken over the unfiltered
  voxel set, in one pass, never iterated.
* Order.  The kept voxels come out in increasing key.  The output is a function of the multiset of input points: it does not depend
  on point order, view order, batching or the number of ranks that held the points.
* File.  Binary little-endian PLY: x y z float, nx ny nz float when there are normals, red green blue uchar when there are colours,
  count int.  MeshLab and CloudCompare read this layout.

* Outliers.  settings["outliers"] = {"radius", "k", "alpha", "min_neighbours"} (cloud_outliers.py, off by default) filters the merged
  cloud between the merge and the file: statistical and radius outlier removal on capped k-nearest-neighbour distances.

Out of scope: weighting by confidence or by nviews; the per-point view lists of the .mvs format; LAS output; feeding the merged
cloud to the DSM.

The kernels are HIP (csrc/cloud.hip); the sort of the keys is torch.sort (plumbing, as in texture.py).  Integer atomicAdd only, so
the cloud is bit-reproducible.

    python -m deep3d_aerial_amd.cloud --fused FOLDER --out C.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --voxel V [--min_points K]
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream

AXIS_MAX = (1 << 21) - 1


class CloudGrid(object):
    """border = [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax] and voxel, checked; n = (n_x, n_y, n_z)."""

    def __init__(self, border, voxel):
        try:
            b = [float(x) for x in border]
        except (TypeError, ValueError):
            raise ValueError("the cloud border must be six numbers Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (got %r)" % (border,))
        if len(b) != 6 or not all(math.isfinite(x) for x in b):
            raise ValueError("the cloud border needs six finite values Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (got %r)" % (border,))
        if not (b[0] < b[1] and b[2] < b[3] and b[4] < b[5]):
            raise ValueError("cloud border %r: every min must be below its max" % (b,))
        try:
            v = float(voxel)
        except (TypeError, ValueError):
            raise ValueError("the cloud voxel must be a number (got %r)" % (voxel,))
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError("the cloud voxel must be finite and > 0 (got %r)" % (voxel,))
        n = [math.ceil((b[2 * a + 1] - b[2 * a]) / v) for a in range(3)]
        if not all(1 <= k <= AXIS_MAX for k in n):
            raise ValueError("a cloud grid of %s voxels: each axis needs 1 .. 2^21 - 1 (border %r, voxel %r)" % (n, b, v))
        self.border, self.voxel, self.n = b, v, tuple(int(k) for k in n)


# ----------------------------------------------------------------------------------------
# what every stage on this grid shares (cloud_outliers, cloud_compare, cloud_register, mesh_compare): the checks of a cloud and
# its keys
# ----------------------------------------------------------------------------------------
def points(t, name, dtype=torch.float32):
    """t checked by name as a [n,3] tensor of dtype (the coordinates of a cloud: fp32) with fewer than 2^31 rows; returns t."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be a [n,3] %s tensor (got %s %s)" % (name, str(dtype).replace("torch.", ""), t.dtype, tuple(t.shape)))
    if int(t.shape[0]) >= 1 << 31:
        raise ValueError("%s has %d points: at most 2^31 - 1" % (name, t.shape[0]))
    return t


def on_gpu(t, name, what):
    """t contiguous; a CPU tensor is refused by name.  what: the stage's verb phrase ("the clouds are compared")."""
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: %s on the GPU (no CPU fallback)" % (name, t.device, what))
    return t.contiguous()


def check_grid(grid):
    if not isinstance(grid, CloudGrid):
        raise TypeError("grid must be a CloudGrid")
    return grid


def point_keys(xyz, grid):
    """xyz [n,3] fp32, checked, contiguous and on a GPU, grid a CloudGrid -> (keys [n] int64, frac [n] int64) of d3d_cloud_keys
    in input order: the package's one call of it.  Queued on the caller's stream; the host reads nothing."""
    n, dev, b = int(xyz.shape[0]), xyz.device, grid.border
    keys = torch.empty((n,), dtype=torch.int64, device=dev)
    frac = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().d3d_cloud_keys(_ptr(xyz) if n else None, n, b[0], b[1], b[2], b[3], b[4], b[5], grid.voxel, _ptr(keys),
                                          _ptr(frac), _stream()), "d3d_cloud_keys")
    return keys, frac


def sorted_keys(xyz, grid):
    """point_keys sorted -> (sorted_keys [n] int64, order [n] int64): the keys in increasing order and the input index of every
    sorted point.  The sort is torch.sort (plumbing)."""
    keys, order = torch.sort(point_keys(xyz, grid)[0])
    return keys, order


def merge_points(xyz, normal, color, grid, min_points=1):
    """xyz [n,3] fp32, normal [n,3] fp32 or None, color [n,3] int32 or None, all on one GPU -> {"xyz" [m,3] fp32, "normal" [m,3] fp32
    or None, "color" [m,3] uint8 or None, "count" [m] int32} (device tensors): the merged cloud of this module's docstring, queued
    on the caller's stream.  The host reads two counts (the voxels and the kept voxels).  CPU tensors are refused."""
    check_grid(grid)
    if not _geom.is_int(min_points, 1, (1 << 31) - 1):
        raise ValueError("min_points must be an integer in 1 .. 2^31 - 1 (got %r)" % (min_points,))
    given = {"xyz": xyz, "normal": normal, "color": color}
    given = {name: t for name, t in given.items() if name == "xyz" or t is not None}
    for name, t in given.items():
        if points(t, name, torch.int32 if name == "color" else torch.float32).shape[0] != xyz.shape[0]:
            raise ValueError("xyz has %d points, %s %d" % (xyz.shape[0], name, t.shape[0]))
    for name, t in given.items():
        given[name] = on_gpu(t, name, "the cloud is merged")
        if t.device != xyz.device:
            raise ValueError("xyz on %s, %s on %s" % (xyz.device, name, t.device))
    xyz, normal, color = given["xyz"], given.get("normal"), given.get("color")
    n, dev = int(xyz.shape[0]), xyz.device
    lib = _lib.load()
    b, v, st = grid.border, grid.voxel, _stream()
    width = 3 + (3 if normal is not None else 0) + (3 if color is not None else 0)
    keys, frac = point_keys(xyz, grid)
    skeys, order = torch.sort(keys)
    del keys
    vox = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_scratch_bytes, n, device=dev)
    _lib.check(lib.d3d_cloud_heads(_ptr(skeys), n, _ptr(scratch), nbytes, _ptr(vox), _ptr(counts[0:1]), st), "d3d_cloud_heads")
    nv = int(counts[0])   # the first host read
    ukeys = torch.empty((nv,), dtype=torch.int64, device=dev)
    count = torch.empty((nv,), dtype=torch.int32, device=dev)
    acc = torch.empty((nv, width), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_cloud_accumulate(_ptr(skeys), _ptr(order), _ptr(vox), _ptr(frac), _ptr(normal), _ptr(color), n, nv,
                                        _ptr(ukeys), _ptr(count), _ptr(acc), st), "d3d_cloud_accumulate")
    del skeys, order, vox, frac
    keep = torch.empty((nv,), dtype=torch.int32, device=dev)
    pos = torch.empty((nv,), dtype=torch.int32, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_scratch_bytes, nv, device=dev)
    _lib.check(lib.d3d_cloud_neighbours(_ptr(ukeys), _ptr(count), nv, grid.n[0], grid.n[1], grid.n[2], int(min_points), _ptr(scratch),
                                        nbytes, _ptr(keep), _ptr(pos), _ptr(counts[1:2]), st), "d3d_cloud_neighbours")
    nk = int(counts[1])   # the second host read
    out = {"xyz": torch.empty((nk, 3), dtype=torch.float32, device=dev),
           "normal": torch.empty((nk, 3), dtype=torch.float32, device=dev) if normal is not None else None,
           "color": torch.empty((nk, 3), dtype=torch.uint8, device=dev) if color is not None else None,
           "count": torch.empty((nk,), dtype=torch.int32, device=dev)}
    _lib.check(lib.d3d_cloud_finalize(_ptr(ukeys), _ptr(count), _ptr(acc), _ptr(keep), _ptr(pos), nv, nk, b[0], b[1], b[2], b[3], b[4],
                                      b[5], v, _ptr(out["xyz"]), _ptr(out["normal"]), _ptr(out["color"]), _ptr(out["count"]), st),
               "d3d_cloud_finalize")
    return out


# ----------------------------------------------------------------------------------------
# the file
# ----------------------------------------------------------------------------------------
def _ply_dtype(normals, colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields + [("count", "<i4")])


def cloud_ply_bytes(xyz, normal, color, count):
    """The bytes of the PLY of a cloud (host arrays or tensors): xyz [m,3] fp32, normal [m,3] fp32 or None, color [m,3] uint8 or
    None, count [m] int32."""
    xyz, count = _geom.host(xyz), _geom.host(count)
    normal = _geom.host(normal) if normal is not None else None
    color = _geom.host(color) if color is not None else None
    m = int(xyz.shape[0])
    if xyz.dtype != np.float32 or xyz.shape != (m, 3) or count.dtype != np.int32 or count.shape != (m,):
        raise ValueError("xyz must be [m,3] float32 and count [m] int32 (got %s %s, %s %s)" % (xyz.shape, xyz.dtype, count.shape, count.dtype))
    if normal is not None and (normal.dtype != np.float32 or normal.shape != (m, 3)):
        raise ValueError("normal must be [%d,3] float32 (got %s %s)" % (m, normal.shape, normal.dtype))
    if color is not None and (color.dtype != np.uint8 or color.shape != (m, 3)):
        raise ValueError("color must be [%d,3] uint8 (got %s %s)" % (m, color.shape, color.dtype))
    dt = _ply_dtype(normal is not None, color is not None)
    rec = np.empty((m,), dt)
    for k, f in enumerate("xyz"):
        rec[f] = xyz[:, k]
    if normal is not None:
        for k, f in enumerate(("nx", "ny", "nz")):
            rec[f] = normal[:, k]
    if color is not None:
        for k, f in enumerate(("red", "green", "blue")):
            rec[f] = color[:, k]
    rec["count"] = count
    return _geom.record_ply_bytes("merged point cloud (deep3d_aerial_amd.cloud)", rec)


def write_cloud_ply(path, xyz, normal, color, count):
    _geom.write_bytes(path, cloud_ply_bytes(xyz, normal, color, count))
    return str(path)


def read_cloud_ply(path):
    """{"xyz", "normal" | None, "color" | None, "count"} as host arrays, of a file write_cloud_ply wrote."""
    with open(str(path), "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("%s: only binary little-endian PLY is read" % path)
    m, props = None, []
    for ln in lines:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            m = int(w[2])
        elif w[:1] == ["element"]:
            raise ValueError("%s: a cloud has only the vertex element (found %r)" % (path, ln))
        elif w[:1] == ["property"]:
            props.append((w[1], w[2]))
    normals, colors = ("float", "nx") in props, ("uchar", "red") in props
    dt = _ply_dtype(normals, colors)
    if m is None or props != [(_geom.PLY_TYPES[dt[f].str], f) for f in dt.names]:
        raise ValueError("%s: not the layout of a merged cloud (properties %r)" % (path, props))
    body = data[end + len(b"end_header\n"):]
    if len(body) != m * dt.itemsize:
        raise ValueError("%s: %d bytes of vertices, %d expected" % (path, len(body), m * dt.itemsize))
    rec = np.frombuffer(body, dt)
    col = lambda names, t: np.ascontiguousarray(np.stack([rec[f] for f in names], 1).astype(t)) if m else np.zeros((0, 3), t)
    return {"xyz": col("xyz", np.float32), "normal": col(("nx", "ny", "nz"), np.float32) if normals else None,
            "color": col(("red", "green", "blue"), np.uint8) if colors else None, "count": np.ascontiguousarray(rec["count"]).astype(np.int32)}


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def check_settings(settings):
    """The settings dict {"path", "border", "voxel", "min_points"} checked: (CloudGrid, min_points); an "outliers" key, when
    there is one, is checked as cloud_outliers.check_settings checks it, on the cloud's border.  No GPU work."""
    if not isinstance(settings, dict):
        raise ValueError("the cloud settings must be a dict (got %r)" % (settings,))
    path = settings.get("path")
    if not path or not str(path).endswith(".ply"):
        raise ValueError("the cloud path must end in .ply (got %r)" % (path,))
    if settings.get("border") is None:
        raise ValueError("the cloud settings need a border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax")
    if settings.get("voxel") is None:
        raise ValueError("the cloud settings need a voxel size")
    grid = CloudGrid(settings["border"], settings["voxel"])
    k = settings.get("min_points", 1)
    k = 1 if k is None else k
    if not _geom.is_int(k, 1, (1 << 31) - 1):
        raise ValueError("cloud min_points must be an integer in 1 .. 2^31 - 1 (got %r)" % (k,))
    if settings.get("outliers") is not None:
        from . import cloud_outliers

        try:
            CloudGrid(grid.border, cloud_outliers.check_settings(settings["outliers"])[0])
        except ValueError as e:
            raise ValueError("cloud outliers: %s" % e)
    return grid, int(k)


def parse_border6(text):
    vals = [float(v) for v in str(text).split(",")]
    if len(vals) != 6:
        raise argparse.ArgumentTypeError("the cloud border needs Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (got %d values)" % len(vals))
    return vals


def add_arguments(ap, prefix=""):
    """The cloud settings as flags (--<prefix>border, ...); used by this module's CLI and by predict (--cloud_*)."""
    ap.add_argument("--%sborder" % prefix, type=parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--%svoxel" % prefix, type=float, default=None, help="voxel size (world units): one point per occupied voxel")
    ap.add_argument("--%smin_points" % prefix, type=int, default=1,
                    help="a voxel is kept when its 3 x 3 x 3 neighbourhood holds at least this many points (1: every voxel)")


def settings_from_args(a, path, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    return {"path": path, "border": g("border"), "voxel": g("voxel"), "min_points": g("min_points")}


def summary(cloud, n_points):
    """{"points", "voxels", "mean_count"}: the input points, the voxels written and the mean support of a written voxel."""
    m = int(cloud["count"].shape[0])
    return {"points": int(n_points), "voxels": m, "mean_count": float(cloud["count"].sum()) / m if m else 0.0}


def build_and_write(xyz, normal, color, settings):
    """merge_points with the settings dict on device tensors, written with write_cloud_ply to settings["path"]:
    (cloud dict, summary).  With settings["outliers"] the merged cloud passes cloud_outliers.filter_cloud on the cloud's border
    before it is written, and the summary (of the written cloud) gains "outliers": the filter's info."""
    grid, k = check_settings(settings)
    cloud = merge_points(xyz, normal, color, grid, k)
    info = None
    if settings.get("outliers") is not None:
        from . import cloud_outliers

        cloud, info = cloud_outliers.filter_cloud(cloud, settings["outliers"], grid.border)
    write_cloud_ply(settings["path"], cloud["xyz"], cloud["normal"], cloud["color"], cloud["count"])
    s = summary(cloud, xyz.shape[0])
    if info is not None:
        s["outliers"] = info
    return cloud, s


def read_fused(folder):
    """(xyz [n,3], normal [n,3] or None) float32: the arrays of every .npz pipeline.save_fused wrote under folder (its scene_<b>
    sub-folders included), in sorted path order.  The normals are None unless every file with points carries them."""
    paths = sorted(os.path.join(r, f) for r, _, fs in os.walk(str(folder)) for f in fs if f.endswith(".npz"))
    if not paths:
        raise FileNotFoundError("no .npz of fused points under %s" % folder)
    xyz, nrm = [], []
    for p in paths:
        with np.load(p) as z:
            xyz.append(np.asarray(z["xyz"], np.float32).reshape(-1, 3))
            nrm.append(np.asarray(z["normal"], np.float32).reshape(-1, 3))
    has = all(len(n) == len(x) for x, n in zip(xyz, nrm))
    return np.concatenate(xyz), np.concatenate(nrm) if has else None


def main(argv=None):
    ap = argparse.ArgumentParser(description="merge the fused points (the .npz files predict --fuse wrote) into one point cloud")
    ap.add_argument("--fused", required=True, help="folder of the fused arrays (<output_folder>/fused)")
    ap.add_argument("--out", required=True, help="the merged cloud (.ply); no colour: the fused arrays store none")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.border is None:
        ap.error("--border is required")
    if a.voxel is None:
        ap.error("--voxel is required")
    settings = settings_from_args(a, a.out)
    try:
        check_settings(settings)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the cloud is merged on the GPU (no CPU fallback)")
    xyz, nrm = read_fused(a.fused)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    _, s = build_and_write(dev(xyz), dev(nrm) if nrm is not None else None, None, settings)
    print("cloud %s: %d points in %d voxels, %.2f points per voxel" % (a.out, s["points"], s["voxels"], s["mean_count"]))
    return a.out


if __name__ == "__main__":
    main()
