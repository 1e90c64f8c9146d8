"""Normals of a point cloud from its own neighbourhoods on the GPU: a plane fitted to the points within a radius (DESIGN.md
§4.34).

The fused cloud gets its normals from the depth maps; a cloud that arrives without them -- a LiDAR reference, a PLY of bare
coordinates -- had none, and the point-to-plane metric of cloud_register needs the reference's.  The rule below is this project's
own; it does not claim to match any tool.

* Inputs.  xyz [n,3] fp32 on one GPU, in any order, duplicates allowed.  border (six values) and radius h > 0 form
  cloud.CloudGrid(border, h): one cell is one radius wide, with the cloud's limits (1 .. 2^21 - 1 cells per axis).
* Keys.  A point is keyed exactly as the cloud keys it (d3d_cloud_keys).  A point that drops (non-finite, or outside the grid) is
  unkeyed: count 0, normal (0, 0, 0), flatness -1; it is nobody's neighbour.
* Neighbours of a keyed point i: every keyed point j of the same cloud, i itself included, in the 3 x 3 x 3 cells around i's cell
  with d2 < h h (strict), d2 = (dx dx + dy dy) + dz dz in fp64, dx = (double)x_i - (double)x_j, each operation rounded once (no
  fused multiply-add).  A point within h lies in those 27 cells, so the window is exact.
* Per neighbour and axis delta_c = llrint(((double)x_jc - (double)x_ic) / h * 1024.0), so |delta_c| <= 1024.
* Ten integer sums, int64: k, the number of neighbours; S1[3] = sum delta; S2[6] = sum delta_r delta_c for rc = xx, xy, xz, yy,
  yz, zz.  k < 2^31 and |S2| < 2^51, so nothing overflows, and integers sum to the same bits in any order.
* Covariance, fp64, each operation rounded once: C_rc = (double)S2_rc - ((double)S1_r * (double)S1_c) / (double)k.  numpy float64
  reproduces it bit for bit.
* Eigenvalues l0 <= l1 <= l2 of C and the unit eigenvector n of l0: six cyclic Jacobi sweeps in fp64 on the device (rotations
  (x, y), (x, z), (y, z) in that order; a zero off-diagonal entry is skipped).  n is a function of the ten integers only, so it too
  is the same bits for any point order.
* Orientation.  n is flipped so that n . up >= 0, up = (0, 0, 1), or (0, 0, -1) with z_down (ortho_mesh's flag for scenes whose Z
  points away from the cameras).  Where n . up == 0 the first non-zero component is made positive.
* Outputs, in input order: normals [n,3] fp32, count [n] int32 = k, flatness [n] int32 = llrint(1024 l0 / (l0 + l1 + l2)): 0 on
  a plane, up to 341 in an isotropic blob.
* Degenerate points -- k < 3, or l2 <= 0, or l1 <= 1e-12 l2 (collinear: the guard cloud_register.solve has on its singular
  values) -- get normal (0, 0, 0), flatness -1 and count k.

Out of scope: orientation by viewpoint or by propagation over the cloud; a k-nearest neighbourhood in place of the radius;
weights.

The search and the fit are HIP (csrc/cloud_normals.hip, on the tile search of csrc/cloud_search.h); the sort of the keys is
torch.sort (plumbing).  No atomics.

    python -m deep3d_aerial_amd.cloud_normals --cloud IN.ply --out OUT.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --radius H
        [--z_down] [--min_count K]
"""
import argparse

import numpy as np
import torch

from . import _geom, _lib, cloud, cloud_compare
from ._geom import ptr as _ptr, stream as _stream

SUMS = 10


def _grid(border, radius):
    try:
        return cloud.CloudGrid(border, radius)
    except ValueError as e:
        raise ValueError("normals grid (border, radius as the voxel): %s" % e)


def _flag(value, name):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError("%s must be True or False (got %r)" % (name, value))
    return bool(value)


def estimate(xyz, border, radius, z_down=False, return_sums=False):
    """xyz [n,3] fp32 on one GPU -> (normals [n,3] fp32, count [n] int32, flatness [n] int32) of the module's docstring, and with
    return_sums the ten sums [n,10] int64 (k, S1 x y z, S2 xx xy xz yy yz zz) as a fourth: device tensors in input order, queued
    on the caller's stream; the host reads nothing.  CPU tensors are refused."""
    z_down, return_sums = _flag(z_down, "z_down"), _flag(return_sums, "return_sums")
    grid = _grid(border, radius)
    xyz = cloud.on_gpu(cloud.points(xyz, "xyz"), "xyz", "the normals are estimated")
    n, dev = int(xyz.shape[0]), xyz.device
    lib = _lib.load()
    sorted_keys, order = cloud.sorted_keys(xyz, grid)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    flatness = torch.empty((n,), dtype=torch.int32, device=dev)
    sums = torch.empty((n, SUMS), dtype=torch.int64, device=dev) if return_sums else None
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_normals_scratch_bytes, n, device=dev)
    pn = (lambda t: _ptr(t) if n else None)
    _lib.check(lib.d3d_cloud_normals(pn(xyz), pn(sorted_keys), pn(order), n, grid.n[0], grid.n[1], grid.n[2], grid.voxel, int(z_down),
                                     _ptr(scratch), nbytes, pn(normals), pn(count), pn(flatness), pn(sums) if return_sums else None,
                                     _stream()), "d3d_cloud_normals")
    return (normals, count, flatness, sums) if return_sums else (normals, count, flatness)


# ----------------------------------------------------------------------------------------
# the file
# ----------------------------------------------------------------------------------------
_COLOUR = ("red", "green", "blue")


def normals_ply_bytes(xyz, normals, color=None):
    """The bytes of a binary little-endian PLY with x y z nx ny nz float per point and, with color [n,3] uint8, red green blue
    uchar, in input order.  Host arrays or tensors."""
    xyz, normals = _geom.host(xyz), _geom.host(normals)
    color = _geom.host(color) if color is not None else None
    n = int(xyz.shape[0])
    if xyz.dtype != np.float32 or xyz.shape != (n, 3) or normals.dtype != np.float32 or normals.shape != (n, 3):
        raise ValueError("xyz and normals must be [n,3] float32 (got %s %s, %s %s)" % (xyz.shape, xyz.dtype, normals.shape, normals.dtype))
    if color is not None and (color.dtype != np.uint8 or color.shape != (n, 3)):
        raise ValueError("color must be [%d,3] uint8 (got %s %s)" % (n, color.shape, color.dtype))
    fields = [(f, "<f4") for f in ("x", "y", "z", "nx", "ny", "nz")] + ([(f, "u1") for f in _COLOUR] if color is not None else [])
    rec = np.zeros((n,), np.dtype(fields))
    for k, f in enumerate(("x", "y", "z")):
        rec[f] = xyz[:, k]
    for k, f in enumerate(("nx", "ny", "nz")):
        rec[f] = normals[:, k]
    if color is not None:
        for k, f in enumerate(_COLOUR):
            rec[f] = color[:, k]
    return _geom.record_ply_bytes("point cloud with estimated normals (deep3d_aerial_amd.cloud_normals)", rec)


def _check_min_count(k):
    if not _geom.is_int(k, 0, (1 << 31) - 1):
        raise ValueError("min_count must be an integer in 0 .. 2^31 - 1 (got %r)" % (k,))
    return int(k)


def main(argv=None):
    ap = argparse.ArgumentParser(description="estimate the normals of a point cloud from its own neighbourhoods")
    ap.add_argument("--cloud", required=True, help="the cloud (.ply, binary little-endian)")
    ap.add_argument("--out", required=True, help="the cloud with x y z nx ny nz, and the input's colour where it has one (.ply)")
    ap.add_argument("--border", type=cloud.parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--radius", type=float, default=None, help="the neighbourhood's radius (world units)")
    ap.add_argument("--z_down", action="store_true", default=False, help="orient the normals towards -Z instead of +Z")
    ap.add_argument("--min_count", type=int, default=0, help="a point with fewer neighbours (itself included) keeps a zero normal")
    a = ap.parse_args(argv)
    if a.border is None:
        ap.error("--border is required")
    if a.radius is None:
        ap.error("--radius is required")
    if not str(a.out).endswith(".ply"):
        ap.error("--out must end in .ply")
    try:
        _grid(a.border, a.radius)
        _check_min_count(a.min_count)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the normals are estimated on the GPU (no CPU fallback)")
    rec = cloud_compare.read_vertex_ply(a.cloud)
    xyz = cloud_compare.vertex_columns(rec, "xyz")
    coloured = all(f in rec.dtype.names and rec.dtype[f].str in ("u1", "|u1") for f in _COLOUR)
    color = cloud_compare.vertex_columns(rec, _COLOUR, np.uint8) if coloured else None
    normals, count, _ = estimate(torch.from_numpy(xyz).cuda(), a.border, a.radius, a.z_down)
    if a.min_count > 0:
        normals = torch.where((count >= a.min_count)[:, None], normals, torch.zeros_like(normals))
    _geom.write_bytes(a.out, normals_ply_bytes(xyz, normals, color))
    with_normal = int((normals != 0).any(1).sum())
    print("cloud %s: %d points, %d with a normal" % (a.out, xyz.shape[0], with_normal))
    return a.out


if __name__ == "__main__":
    main()
