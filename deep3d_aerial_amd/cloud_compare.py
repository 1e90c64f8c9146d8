"""Comparison of two point clouds on the GPU by capped nearest-neighbour distances: accuracy, completeness and F-score of a
reconstructed cloud against a reference cloud (LiDAR, or another reconstruction).

Aerial multi-view stereo is judged by the distance from each reconstructed point to the reference (accuracy), the distance from
each reference point to the reconstruction (completeness), the share of each under a threshold, and the F-score of the two.  The
rule below is this project's own; it does not claim to match any tool.

* Inputs.  Query points Q [nq,3] fp32 and target points T [nt,3] fp32 on one GPU, in any order, duplicates allowed.  border (six
  values) and a cap h > 0 form cloud.CloudGrid(border, h): one cell is one cap wide, with the cloud's limits (1 .. 2^21 - 1 cells
  per axis).
* Keys.  Both clouds are keyed exactly as the cloud keys its points (d3d_cloud_keys with voxel = h, the single copy of the rule).
  A point that drops (non-finite, or outside the grid) is unkeyed: as a query it gets e = -1, idx = -1 and enters no count; as a
  target it is nobody's neighbour.
* Per keyed query i, over every keyed target j:
  - d2 = (dx dx + dy dy) + dz dz in fp64, dx = (double)q_x - (double)t_x, each operation rounded once (no fused multiply-add).
  - cap2 = h h.
  - The nearest is the j with d2 < cap2 that minimises (d2, j) lexicographically, j the index in T's input order: of equally
    distant targets the lowest input index wins.
  - When there is a nearest: idx_i = j and e_i = min(1024, llrint(sqrt(d2) / h * 1024.0)), the outliers' e; fp64 sqrt and division
    are correctly rounded.
  - When there is none: idx_i = -1 and e_i = 1024.
  - e does not decrease with d2, so e_i does not depend on the tie rule; only idx_i does.
  - A target within h lies in the 3 x 3 x 3 cells around the query's cell, so the 27-cell window is exact under the cap.
* Histogram.  hist int64 [1026], zeroed by the call: hist[e], e in 0 .. 1024, counts the keyed queries that found a neighbour with
  that e; hist[1025] counts the keyed queries that found none.  m = sum(hist) is the number of keyed queries.
* Statistics: host Python on the two histograms, exact integers until the last division.  A is the evaluated cloud, B the
  reference, m_A and m_B their keyed counts, hist_A of A queried against B and hist_B of B queried against A;
  cum[t] = hist[0] + .. + hist[t].
  - The distance of a bin e is min(e, 1024) / 1024 * h: a query that found nothing counts the cap.
  - A threshold tau becomes t = floor(tau / h * 1024 + 0.5); it must give 1 <= t <= 1023, else ValueError (a threshold at the cap
    would count the queries that found nothing).
  - accuracy P = cum_A[t] / m_A, completeness R = cum_B[t] / m_B,
    fscore = 2 P R / (P + R) = 2 cum_A[t] cum_B[t] / (cum_A[t] m_B + cum_B[t] m_A), and 0 when that denominator is 0.
  - Per direction: mean = S1 / (1024 m) * h and rms = sqrt(S2 / (1024^2 m)) * h with S1 = sum min(e, 1024) hist[e] and
    S2 = sum min(e, 1024)^2 hist[e] exact integers; for p in (50, 90, 95) the distance of the smallest e with
    cum[e] >= (p m + 99) // 100; "points" (the input points), "keyed" = m and "beyond" = hist[1025].
  - m = 0 gives zeros without dividing.
* Output.  e int32 [nq] and idx int32 [nq] in input order, hist, and the dict of stats().  e and hist depend only on the two
  multisets of points; idx follows a permutation of T.

Out of scope: a shift of large coordinates before the fp32 rounding; cloud-to-mesh distance; normals or colour in the comparison;
an uncapped search.  The two clouds must be in one frame: cloud_register finds the rigid transform, and
--transform applies it here.  Ground truth is not an input of a
reconstruction run: pipeline.predict_and_fuse and predict have no key or flag for this.

The search is HIP (csrc/cloud_compare.hip); the sort of the keys is torch.sort (plumbing).  Integer atomicAdd only, so the result
is bit-reproducible.

    python -m deep3d_aerial_amd.cloud_compare --cloud A.ply --reference B.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --max_dist H
        --threshold T[,T...] [--transform T.txt] [--json R.json] [--out_accuracy EA.ply] [--out_completeness EB.ply]

--transform: a 4 x 4 transform as cloud_register writes it; the evaluated cloud goes through cloud_register.apply before anything
else, and --out_accuracy carries the moved coordinates.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import _geom, _lib, cloud
from ._geom import ptr as _ptr, stream as _stream

CAP = 1024
BINS = CAP + 2
PERCENTILES = (50, 90, 95)


# ----------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------
_VERB = "the clouds are compared"


def prepare(xyz, grid):
    """xyz [n,3] fp32 on one GPU, grid = CloudGrid(border, cap) -> (sorted_keys [n] int64, order [n] int64): the keys of
    d3d_cloud_keys with voxel = the cap, sorted, and the input index of every sorted point (cloud.sorted_keys).  A cloud is
    prepared once for both directions of a comparison.  Queued on the caller's stream; the host reads nothing."""
    cloud.check_grid(grid)
    return cloud.sorted_keys(cloud.on_gpu(cloud.points(xyz, "xyz"), "xyz", _VERB), grid)


def _prepared(p, xyz, grid, name):
    if p is None:
        return prepare(xyz, grid)
    n = int(xyz.shape[0])
    if not (isinstance(p, (tuple, list)) and len(p) == 2 and all(isinstance(t, torch.Tensor) for t in p)):
        raise TypeError("%s must be the (sorted_keys, order) of prepare()" % name)
    for t in p:
        if t.dtype != torch.int64 or tuple(t.shape) != (n,) or t.device != xyz.device:
            raise ValueError("%s must be two [%d] int64 tensors on %s (got %s %s on %s)" % (name, n, xyz.device, t.dtype, tuple(t.shape), t.device))
    return p[0].contiguous(), p[1].contiguous()


def nearest(query, target, grid, query_prepared=None, target_prepared=None):
    """query [nq,3] fp32 and target [nt,3] fp32 on one GPU, grid = CloudGrid(border, cap) -> (e [nq] int32, idx [nq] int32,
    hist [1026] int64) of the module's docstring: device tensors queued on the caller's stream; the host reads nothing.
    query_prepared / target_prepared: what prepare() returned for that cloud on this grid.  CPU tensors are refused.  The two
    clouds must not share memory (compare a cloud with a clone of itself)."""
    cloud.check_grid(grid)
    query, target = cloud.points(query, "query"), cloud.points(target, "target")
    query, target = cloud.on_gpu(query, "query", _VERB), cloud.on_gpu(target, "target", _VERB)
    if query.device != target.device:
        raise ValueError("query is on %s and target on %s: both clouds must be on one GPU" % (query.device, target.device))
    nq, nt, dev = int(query.shape[0]), int(target.shape[0]), query.device
    q_keys, q_order = _prepared(query_prepared, query, grid, "query_prepared")
    t_keys, t_order = _prepared(target_prepared, target, grid, "target_prepared")
    lib = _lib.load()
    e = torch.empty((nq,), dtype=torch.int32, device=dev)
    idx = torch.empty((nq,), dtype=torch.int32, device=dev)
    hist = torch.zeros((BINS,), dtype=torch.int64, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_compare_scratch_bytes, nq, nt, device=dev)
    pq = (lambda t: _ptr(t) if nq else None)
    pt = (lambda t: _ptr(t) if nt else None)
    _lib.check(lib.d3d_cloud_compare_nearest(pq(query), pq(q_keys), pq(q_order), nq, pt(target), pt(t_keys), pt(t_order), nt, grid.n[0],
                                             grid.n[1], grid.n[2], grid.voxel, _ptr(scratch), nbytes, pq(e), pq(idx), _ptr(hist), _stream()),
               "d3d_cloud_compare_nearest")
    return e, idx, hist


# ----------------------------------------------------------------------------------------
# the statistics (host only)
# ----------------------------------------------------------------------------------------
def _hist(h, name):
    if isinstance(h, torch.Tensor):
        h = h.tolist()
    h = [int(v) for v in h]
    if len(h) != BINS or min(h) < 0:
        raise ValueError("%s must hold %d counts >= 0 (got %d)" % (name, BINS, len(h)))
    return h


def check_max_dist(max_dist):
    """The cap as a float; ValueError unless it is a finite number > 0."""
    if not _geom.is_real(max_dist, above=0):
        raise ValueError("max_dist must be finite and > 0 (got %r)" % (max_dist,))
    return float(max_dist)


def threshold_bin(tau, max_dist):
    """t = floor(tau / h * 1024 + 0.5) of a threshold tau under the cap h; ValueError unless 1 <= t <= 1023."""
    h = check_max_dist(max_dist)
    if not _geom.is_real(tau):
        raise ValueError("a threshold must be a finite number (got %r)" % (tau,))
    t = math.floor(float(tau) / h * 1024.0 + 0.5)
    if not 1 <= t <= CAP - 1:
        raise ValueError("threshold %r under max_dist %r is bin %d: it must lie in 1 .. 1023 (a threshold at the cap would count the "
                         "points that found no neighbour)" % (tau, max_dist, t))
    return int(t)


def check_thresholds(thresholds, max_dist):
    """[(tau, bin)] of one threshold or a sequence of them under the cap max_dist, each through threshold_bin."""
    try:
        taus = list(thresholds)
    except TypeError:
        taus = [thresholds]
    if not taus:
        raise ValueError("at least one threshold is needed")
    return [(float(tau), threshold_bin(tau, max_dist)) for tau in taus]


def _direction(hist, h, points):
    m = sum(hist)
    cum, c = [], 0
    for v in hist:
        c += v
        cum.append(c)
    s1 = sum(min(e, CAP) * v for e, v in enumerate(hist))
    s2 = sum(min(e, CAP) ** 2 * v for e, v in enumerate(hist))
    out = {"points": points, "keyed": m, "beyond": hist[BINS - 1], "mean": s1 / (CAP * m) * h if m else 0.0,
           "rms": math.sqrt(s2 / (CAP * CAP * m)) * h if m else 0.0}
    for p in PERCENTILES:
        need = (p * m + 99) // 100
        e = next(k for k in range(BINS) if cum[k] >= need) if m else 0
        out["p%d" % p] = min(e, CAP) / CAP * h
    return out, cum, m


def stats(hist_cloud, hist_reference, max_dist, thresholds, points=None):
    """The statistics of the module's docstring from the two histograms: hist_cloud of the evaluated cloud queried against the
    reference, hist_reference of the reference queried against the cloud (lists, arrays or tensors of 1026 counts).  Host only,
    no GPU needed.  points: (points of the cloud, points of the reference) for the "points" entries, else they are None.
    -> {"max_dist": h, "cloud": {...}, "reference": {...}, "thresholds": [{"threshold", "bin", "accuracy", "completeness",
    "fscore"}, ...]} with {"points", "keyed", "beyond", "mean", "rms", "p50", "p90", "p95"} per direction."""
    h = check_max_dist(max_dist)
    taus = check_thresholds(thresholds, h)
    ha, hb = _hist(hist_cloud, "hist_cloud"), _hist(hist_reference, "hist_reference")
    pa, pb = (None, None) if points is None else (int(points[0]), int(points[1]))
    a, cum_a, ma = _direction(ha, h, pa)
    b, cum_b, mb = _direction(hb, h, pb)
    rows = []
    for tau, t in taus:
        ca, cb = cum_a[t], cum_b[t]
        den = ca * mb + cb * ma
        rows.append({"threshold": tau, "bin": t, "accuracy": ca / ma if ma else 0.0, "completeness": cb / mb if mb else 0.0,
                     "fscore": 2 * ca * cb / den if den else 0.0})
    return {"max_dist": h, "cloud": a, "reference": b, "thresholds": rows}


def compare(cloud_xyz, reference_xyz, border, max_dist, thresholds):
    """(result, {"cloud": (e, idx), "reference": (e, idx)}): the dict of stats() for the cloud [n,3] fp32 against the reference
    [n,3] fp32 (device tensors on one GPU), and per direction the device tensors of nearest().  The host reads the two histograms
    in one read."""
    taus = check_thresholds(thresholds, check_max_dist(max_dist))
    try:
        grid = cloud.CloudGrid(border, max_dist)
    except ValueError as e:
        raise ValueError("compare grid (border, max_dist as the voxel): %s" % e)
    pa, pb = prepare(cloud_xyz, grid), prepare(reference_xyz, grid)
    ea, ia, ha = nearest(cloud_xyz, reference_xyz, grid, pa, pb)
    eb, ib, hb = nearest(reference_xyz, cloud_xyz, grid, pb, pa)
    both = torch.stack([ha, hb]).tolist()   # the one read
    result = stats(both[0], both[1], grid.voxel, [tau for tau, _ in taus], (int(cloud_xyz.shape[0]), int(reference_xyz.shape[0])))
    return result, {"cloud": (ea, ia), "reference": (eb, ib)}


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
                "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8",
                "float64": "<f8"}


def read_vertex_ply(path):
    """The vertices of a binary little-endian PLY as a structured host array, one field per scalar property, named and typed as
    the file has them.  The vertex element must be the first one; its scalar properties may be of any PLY scalar type; x, y and z
    must be float or double.  Later elements (faces) are skipped.  ASCII and big-endian files are refused by name."""
    with open(str(path), "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").split("\n")]
    fmt = [w for w in lines if w[:1] == ["format"]]
    if len(fmt) != 1 or len(fmt[0]) < 2:
        raise ValueError("%s: a PLY header needs one format line" % path)
    if fmt[0][1] == "ascii":
        raise ValueError("%s: ASCII PLY is not read (only binary little-endian)" % path)
    if fmt[0][1] == "binary_big_endian":
        raise ValueError("%s: big-endian PLY is not read (only binary little-endian)" % path)
    if fmt[0][1] != "binary_little_endian":
        raise ValueError("%s: unknown PLY format %r" % (path, fmt[0][1]))
    elements = [k for k, w in enumerate(lines) if w[:1] == ["element"]]
    if not elements or lines[elements[0]][1:2] != ["vertex"] or len(lines[elements[0]]) != 3:
        raise ValueError("%s: the vertex element must be the first element of the file" % path)
    try:
        m = int(lines[elements[0]][2])
    except ValueError:
        m = -1
    if m < 0:
        raise ValueError("%s: bad vertex count %r" % (path, lines[elements[0]][2]))
    fields = []
    for w in lines[elements[0] + 1:elements[1] if len(elements) > 1 else len(lines)]:
        if w[:1] != ["property"]:
            continue
        if len(w) != 3 or w[1] not in _PLY_SCALARS:
            raise ValueError("%s: vertex property %r is not a scalar of a PLY type" % (path, " ".join(w)))
        if w[2] in [name for name, _ in fields]:
            raise ValueError("%s: vertex property %r is given twice" % (path, w[2]))
        fields.append((w[2], _PLY_SCALARS[w[1]]))
    names = dict(fields)
    for axis in "xyz":
        if axis not in names:
            raise ValueError("%s: the vertex element has no property %s" % (path, axis))
        if names[axis] not in ("<f4", "<f8"):
            raise ValueError("%s: vertex property %s must be float or double" % (path, axis))
    dt = np.dtype(fields)
    body = end + len(b"end_header\n")
    if len(data) - body < m * dt.itemsize:
        raise ValueError("%s: %d bytes after the header, %d vertices need %d" % (path, len(data) - body, m, m * dt.itemsize))
    return np.frombuffer(data, dt, count=m, offset=body)


def vertex_columns(rec, names, dtype=np.float32):
    """The properties `names` of read_vertex_ply's records as one contiguous [n, len(names)] array of dtype."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.stack([rec[a].astype(dtype) for a in names], 1)) if len(rec) else np.zeros((0, len(names)), dtype)


def read_xyz_ply(path, normals=False):
    """xyz [n,3] float32 (a host array) of the vertices of a PLY that read_vertex_ply reads (double is rounded to fp32); other
    properties are skipped.  With normals: (xyz, normal), normal [n,3] float32 from nx ny nz where the file has all three as float
    or double, else None."""
    rec = read_vertex_ply(path)
    if not normals:
        return vertex_columns(rec, "xyz")
    has = all(a in rec.dtype.names and rec.dtype[a].str in ("<f4", "<f8") for a in ("nx", "ny", "nz"))
    return vertex_columns(rec, "xyz"), vertex_columns(rec, ("nx", "ny", "nz")) if has else None


_ERROR_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("e", "<i4")])


def error_cloud_bytes(xyz, e):
    """The bytes of an error cloud: every point of xyz [n,3] fp32 in input order as x y z float, red green blue uchar, e int, with
    red = min(255, e >> 1), green = min(255, (1024 - e) >> 1), blue = 0; an unkeyed point (e = -1) is grey (128, 128, 128).
    Host arrays or tensors."""
    xyz, e = _geom.host(xyz), _geom.host(e)
    n = int(xyz.shape[0])
    if xyz.dtype != np.float32 or xyz.shape != (n, 3) or e.dtype != np.int32 or e.shape != (n,):
        raise ValueError("xyz must be [n,3] float32 and e [n] int32 (got %s %s, %s %s)" % (xyz.shape, xyz.dtype, e.shape, e.dtype))
    if n and (e.min() < -1 or e.max() > CAP):
        raise ValueError("e must lie in -1 .. 1024")
    rec = np.empty((n,), _ERROR_DTYPE)
    for k, f in enumerate("xyz"):
        rec[f] = xyz[:, k]
    keyed = e >= 0
    rec["red"] = np.where(keyed, np.minimum(255, e >> 1), 128)
    rec["green"] = np.where(keyed, np.minimum(255, (CAP - e) >> 1), 128)
    rec["blue"] = np.where(keyed, 0, 128)
    rec["e"] = e
    return _geom.record_ply_bytes("error cloud (deep3d_aerial_amd.cloud_compare)", rec)


# ----------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------
def parse_thresholds(text):
    try:
        vals = [float(v) for v in str(text).split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("--threshold needs T[,T...] (got %r)" % (text,))
    return vals


def main(argv=None):
    ap = argparse.ArgumentParser(description="accuracy, completeness and F-score of a point cloud against a reference cloud")
    ap.add_argument("--cloud", default=None, help="the evaluated cloud (.ply, binary little-endian)")
    ap.add_argument("--reference", default=None, help="the reference cloud, or a mesh whose vertices serve (.ply)")
    ap.add_argument("--border", type=cloud.parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--max_dist", type=float, default=None, help="the cap of the distances (world units); further points count the cap")
    ap.add_argument("--threshold", type=parse_thresholds, default=None, help="T[,T...]: the distances under which a point counts")
    ap.add_argument("--json", default=None, help="write the result here too (.json)")
    ap.add_argument("--out_accuracy", default=None, help="the evaluated cloud coloured by its distance to the reference (.ply)")
    ap.add_argument("--out_completeness", default=None, help="the reference coloured by its distance to the evaluated cloud (.ply)")
    from . import cloud_register   # (it imports this module)

    cloud_register.add_transform_argument(ap)
    a = ap.parse_args(argv)
    for flag in ("cloud", "reference", "border", "max_dist", "threshold"):
        if getattr(a, flag) is None:
            ap.error("--%s is required" % flag)
    for flag in ("out_accuracy", "out_completeness"):
        if getattr(a, flag) is not None and not str(getattr(a, flag)).endswith(".ply"):
            ap.error("--%s must end in .ply" % flag)
    if a.json is not None and not str(a.json).endswith(".json"):
        ap.error("--json must end in .json")
    outs = [os.path.abspath(str(p)) for p in (a.json, a.out_accuracy, a.out_completeness) if p is not None]
    if len(set(outs)) != len(outs):
        ap.error("two of --json, --out_accuracy and --out_completeness name the same file")
    if set(outs) & {os.path.abspath(str(a.cloud)), os.path.abspath(str(a.reference))}:
        ap.error("an output would overwrite an input cloud")
    cloud_register.check_transform_argument(ap, a.transform, {os.path.abspath(str(a.cloud)), os.path.abspath(str(a.reference))}, outs)
    try:
        check_thresholds(a.threshold, check_max_dist(a.max_dist))
        cloud.CloudGrid(a.border, a.max_dist)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the clouds are compared on the GPU (no CPU fallback)")
    xa, xb = read_xyz_ply(a.cloud), read_xyz_ply(a.reference)
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    if a.transform is not None:   # the evaluated cloud moves first; the error cloud carries the moved coordinates
        da = cloud_register.apply(da, cloud_register.read_transform(a.transform))
        xa = da.cpu().numpy()
    result, found = compare(da, db, a.border, a.max_dist, a.threshold)
    line = json.dumps(result)
    if a.out_accuracy is not None:
        _geom.write_bytes(a.out_accuracy, error_cloud_bytes(xa, found["cloud"][0]))
    if a.out_completeness is not None:
        _geom.write_bytes(a.out_completeness, error_cloud_bytes(xb, found["reference"][0]))
    if a.json is not None:
        _geom.write_bytes(a.json, (line + "\n").encode("ascii"))
    print(line)
    return result


if __name__ == "__main__":
    main()
