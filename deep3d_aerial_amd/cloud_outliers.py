"""Outlier removal on a point cloud -- the merged cloud of cloud.py, or raw fused points -- by capped k-nearest-neighbour
distances: a statistical test on the mean distance to the k nearest neighbours and a count of the neighbours within a radius
(DESIGN.md §4.28).

cloud.py's min_points counts the points of a 3 x 3 x 3 voxel neighbourhood and is blind to distance: a floater two voxels above a
roof sits next to occupied voxels and survives.  The two tests here are the cleaning filters of every point-cloud tool (statistical
and radius outlier removal).  The rule below is this project's own; it does not claim to match any tool.

* Inputs.  xyz [n,3] fp32 on one GPU, in any order, duplicates allowed.  border (six values) and radius h > 0 form
  cloud.CloudGrid(border, h): one cell is one radius wide, with the cloud's limits (1 .. 2^21 - 1 cells per axis).  k in 1 .. 32.
  alpha: a finite float >= 0, or None, which turns the statistical test off.  min_neighbours M in 0 .. 2^31 - 1; 0 is off.  At
  least one of the two tests must be on, else ValueError.
* Keys.  A point is keyed exactly as the cloud keys it (d3d_cloud_keys, the single copy of the rule).  A point that drops
  (non-finite, or outside the grid) is unkeyed: D = -1, nn = -1, keep = 0; it is nobody's neighbour and not in the statistics.
* Per keyed point i.  Every other keyed point j is a candidate; j != i by index, so a duplicate of i at distance 0 counts.
  - d2 = (dx dx + dy dy) + dz dz in fp64, dx = (double)x_i - (double)x_j, each operation rounded once (no fused multiply-add).
  - cap2 = h h.
  - e_ij = 1024 when d2 >= cap2, else min(1024, llrint(sqrt(d2) / h * 1024.0)); fp64 sqrt and division are correctly rounded.
  - nn_i = the number of j with d2 < cap2.
  - D_i = the sum of the k smallest e_ij; a missing neighbour, when there are fewer than k candidates, counts 1024.  D_i is an
    integer in 0 .. 1024 k, so neither the order nor the tie-breaking of the selection can change it.
  - A point within h lies in the 3 x 3 x 3 cells around i's cell, and anything further adds exactly 1024, which is what a missing
    neighbour adds: the 27-cell window gives the exact unbounded k-nearest answer under the cap.
* Statistics, over the m keyed points: S1 = sum D and S2 = sum D^2 as int64 (D <= 2^15 and m < 2^31 keep S2 below 2^61).  The host
  reads m, S1 and S2 in one read and computes, in Python, mu = S1 / m, sigma = sqrt(m S2 - S1 S1) / m with the radicand an exact
  integer, and T = floor(mu + alpha sigma).  keep_i = (alpha is None or D_i <= T) and nn_i >= M.  One pass, never iterated.  m = 0
  gives an empty result without dividing.
* Output.  D int32 [n], nn int32 [n] and keep bool [n], in input order, and {"points": n, "keyed": m, "kept", "mu", "sigma",
  "threshold"}.  A point's three values depend only on the multiset of points, not on their order.

The search and the selection are HIP (csrc/cloud_outliers.hip); the sort of the keys is torch.sort and the two comparisons of the
mask are torch (plumbing).  Integer atomicAdd only, so the result is bit-reproducible.

    python -m deep3d_aerial_amd.cloud_outliers --cloud IN.ply --out OUT.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --radius H
        [--k 8] [--alpha 2.0 | --no_alpha] [--min_neighbours M]
"""
import argparse
import math

import numpy as np
import torch

from . import _geom, _lib, cloud
from ._geom import ptr as _ptr, stream as _stream

K_MAX = 32
CAP = 1024
DEFAULT_K, DEFAULT_ALPHA = 8, 2.0
_KEYS = ("radius", "k", "alpha", "min_neighbours")


def _check_k(k):
    if not _geom.is_int(k, 1, K_MAX):
        raise ValueError("outlier k must be an integer in 1 .. %d (got %r)" % (K_MAX, k))
    return int(k)


def _check_tests(alpha, min_neighbours):
    if alpha is not None:
        if not _geom.is_real(alpha, at_least=0):
            raise ValueError("outlier alpha must be a finite number >= 0, or None (got %r)" % (alpha,))
        alpha = float(alpha)
    if not _geom.is_int(min_neighbours, 0, (1 << 31) - 1):
        raise ValueError("outlier min_neighbours must be an integer in 0 .. 2^31 - 1 (got %r)" % (min_neighbours,))
    if alpha is None and int(min_neighbours) == 0:
        raise ValueError("outlier removal with alpha None and min_neighbours 0: at least one of the two tests must be on")
    return alpha, int(min_neighbours)


def point_distances(xyz, grid, k):
    """xyz [n,3] fp32 on one GPU, grid = CloudGrid(border, radius), k in 1 .. 32 -> (D [n] int32, nn [n] int32, sums [3] int64 =
    m, S1, S2), device tensors queued on the caller's stream; the host reads nothing.  CPU tensors are refused."""
    cloud.check_grid(grid)
    k = _check_k(k)
    xyz = cloud.on_gpu(cloud.points(xyz, "xyz"), "xyz", "the outliers are found")
    n, dev = int(xyz.shape[0]), xyz.device
    lib = _lib.load()
    h, st = grid.voxel, _stream()
    sorted_keys, order = cloud.sorted_keys(xyz, grid)
    dist = torch.empty((n,), dtype=torch.int32, device=dev)
    nn = torch.empty((n,), dtype=torch.int32, device=dev)
    sums = torch.zeros((3,), dtype=torch.int64, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_outliers_scratch_bytes, n, device=dev)
    _lib.check(lib.d3d_cloud_outliers_distances(_ptr(xyz) if n else None, _ptr(sorted_keys), _ptr(order), n, grid.n[0], grid.n[1], grid.n[2],
                                                h, k, _ptr(scratch), nbytes, _ptr(dist), _ptr(nn), _ptr(sums), st),
               "d3d_cloud_outliers_distances")
    return dist, nn, sums


def threshold(m, s1, s2, alpha):
    """(mu, sigma, T) of the module's docstring from the three integer sums; T is None when alpha is; (0.0, 0.0, T of them) for
    m = 0."""
    m, s1, s2 = int(m), int(s1), int(s2)
    mu = s1 / m if m else 0.0
    sigma = math.sqrt(m * s2 - s1 * s1) / m if m else 0.0
    return mu, sigma, None if alpha is None else int(math.floor(mu + alpha * sigma))


def outlier_mask(xyz, border, radius, k=DEFAULT_K, alpha=DEFAULT_ALPHA, min_neighbours=0):
    """(keep [n] bool on xyz's device, info) of the module's docstring.  The host reads the three sums in one read, then the
    number of kept points."""
    alpha, min_neighbours = _check_tests(alpha, min_neighbours)
    k = _check_k(k)
    grid = _grid(border, radius)
    dist, nn, sums = point_distances(xyz, grid, k)
    m, s1, s2 = sums.tolist()   # the one read of the statistics
    mu, sigma, T = threshold(m, s1, s2, alpha)
    keep = nn >= min_neighbours if min_neighbours > 0 else nn >= 0
    if T is not None:
        keep = keep & (dist >= 0) & (dist <= T)
    kept = int(keep.sum()) if m else 0
    return keep, {"points": int(xyz.shape[0]), "keyed": int(m), "kept": kept, "mu": mu, "sigma": sigma, "threshold": T}


def _grid(border, radius):
    try:
        return cloud.CloudGrid(border, radius)
    except ValueError as e:
        raise ValueError("outlier grid (border, radius as the voxel): %s" % e)


def check_settings(settings):
    """The settings dict {"radius", "k", "alpha", "min_neighbours"} checked: (radius, k, alpha, min_neighbours) with the defaults
    k = 8, alpha = 2.0 (None: the statistical test off), min_neighbours = 0 filled in.  A "border" key may ride along
    (filter_cloud); any other key is an error.  No GPU work."""
    if not isinstance(settings, dict):
        raise ValueError("the outlier settings must be a dict (got %r)" % (settings,))
    unknown = sorted(set(settings) - set(_KEYS) - {"border"})
    if unknown:
        raise ValueError("unknown outlier settings %r (known: %s)" % (unknown, ", ".join(_KEYS)))
    h = settings.get("radius")
    if not _geom.is_real(h, above=0):
        raise ValueError("the outlier radius must be finite and > 0 (got %r)" % (h,))
    k = settings.get("k")
    m = settings.get("min_neighbours")
    alpha, m = _check_tests(settings.get("alpha", DEFAULT_ALPHA), 0 if m is None else m)
    return float(h), _check_k(DEFAULT_K if k is None else k), alpha, m


def filter_cloud(cloud_dict, settings, border=None):
    """The cloud dict of cloud.merge_points (device tensors "xyz", "normal" | None, "color" | None, "count") with every array
    masked by outlier_mask on its xyz, the order kept: (cloud dict, info).  border: the grid's six values, else
    settings["border"]."""
    h, k, alpha, m = check_settings(settings)
    border = settings.get("border") if border is None else border
    if border is None:
        raise ValueError("the outlier removal needs a border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax")
    if not isinstance(cloud_dict, dict) or sorted(cloud_dict) != ["color", "count", "normal", "xyz"]:
        raise ValueError("a cloud is the dict of merge_points: xyz, normal, color, count")
    for name, t in cloud_dict.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor or None" % name)
        if t is not None and t.shape[0] != cloud_dict["xyz"].shape[0]:
            raise ValueError("xyz has %d points, %s %d" % (cloud_dict["xyz"].shape[0], name, t.shape[0]))
    keep, info = outlier_mask(cloud_dict["xyz"], border, h, k, alpha, m)
    return {name: (None if t is None else t.to(keep.device)[keep].contiguous()) for name, t in cloud_dict.items()}, info


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix=""):
    """The outlier settings as flags (--<prefix>radius, ...); used by this module's CLI and by predict (--cloud_outlier_*)."""
    ap.add_argument("--%sradius" % prefix, type=float, default=None,
                    help="remove outliers from the cloud: the neighbour radius (world units); distances are capped at it")
    ap.add_argument("--%sk" % prefix, type=int, default=None, help="the number of nearest neighbours, 1 .. %d (default %d)" % (K_MAX, DEFAULT_K))
    ap.add_argument("--%salpha" % prefix, type=float, default=None,
                    help="keep a point when its k-nearest distance sum is at most mean + alpha x deviation (default %g)" % DEFAULT_ALPHA)
    ap.add_argument("--%sno_alpha" % prefix, action="store_true", default=False, help="turn the statistical test off")
    ap.add_argument("--%smin_neighbours" % prefix, type=int, default=None,
                    help="keep a point when at least this many others lie within the radius (default 0: off)")


def given(a, prefix=""):
    """The names of the outlier flags other than the radius that the command line set."""
    g = lambda k: getattr(a, prefix + k)
    return [n for n in ("k", "alpha", "min_neighbours") if g(n) is not None] + (["no_alpha"] if g("no_alpha") else [])


def settings_from_args(a, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    if g("no_alpha") and g("alpha") is not None:
        raise ValueError("--%salpha and --%sno_alpha exclude each other" % (prefix, prefix))
    alpha = None if g("no_alpha") else (DEFAULT_ALPHA if g("alpha") is None else g("alpha"))
    return {"radius": g("radius"), "k": DEFAULT_K if g("k") is None else g("k"), "alpha": alpha,
            "min_neighbours": 0 if g("min_neighbours") is None else g("min_neighbours")}


def main(argv=None):
    ap = argparse.ArgumentParser(description="remove the outliers of a merged point cloud (a .ply deep3d_aerial_amd.cloud wrote)")
    ap.add_argument("--cloud", required=True, help="the cloud to clean (.ply)")
    ap.add_argument("--out", required=True, help="the cleaned cloud (.ply), in the same layout and order")
    ap.add_argument("--border", type=cloud.parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.border is None:
        ap.error("--border is required")
    if a.radius is None:
        ap.error("--radius is required")
    if not str(a.out).endswith(".ply"):
        ap.error("--out must end in .ply")
    try:
        settings = settings_from_args(a)
        check_settings(settings)
        _grid(a.border, a.radius)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the outliers are found on the GPU (no CPU fallback)")
    c = cloud.read_cloud_ply(a.cloud)
    dev = {name: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for name, v in c.items()}
    out, info = filter_cloud(dev, settings, a.border)
    cloud.write_cloud_ply(a.out, out["xyz"], out["normal"], out["color"], out["count"])
    print("cloud %s: kept %d of %d points, dropped %d (threshold %s, mean %.2f, deviation %.2f)"
          % (a.out, info["kept"], info["points"], info["points"] - info["kept"], info["threshold"], info["mu"], info["sigma"]))
    return a.out


if __name__ == "__main__":
    main()
