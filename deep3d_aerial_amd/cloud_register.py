"""Rigid registration of a point cloud to a reference cloud on the GPU (iterative closest point) before the two are compared
(DESIGN.md §4.31).

A reconstruction from aerial cameras sits a few decimetres and a fraction of a degree off a LiDAR survey (the GPS/INS solution, the
datum, the bundle adjustment).  At a threshold of a few centimetres the accuracy, completeness and F-score of cloud_compare then
measure that offset, not the reconstruction: every evaluation protocol for aerial multi-view stereo registers first.  The rule below
is this project's own; it does not claim to match any tool.

* Inputs.  The evaluated cloud P [n,3] and the reference Q [m,3], both fp32 on one GPU, in any order.  A border of six values.  A
  schedule of caps h_1 > h_2 > ... > h_S > 0, one stage per cap, coarse to fine.  An initial transform T_0, a 4 x 4 fp64 matrix
  whose last row is 0 0 0 1 (default: the identity).  max_iterations per stage (default 50, at least 1).  tolerance in world units
  (default: one bin of the stage, h_s / 1024).  Optionally max_pair_dist: per stage it becomes a bin through
  cloud_compare.threshold_bin(max_pair_dist, h_s); without it every found pair counts.
* Transform (d3d_cloud_transform).  For each output row r:
    p'_r = (float)(((T[r][0] * (double)x + T[r][1] * (double)y) + T[r][2] * (double)z) + T[r][3])
  - Each operation is fp64 and rounded once (no fused multiply-add); the result is rounded once to fp32.
  - A non-finite input gives whatever that arithmetic gives.  The keys drop the point later.
  - Every iteration transforms the ORIGINAL P by the accumulated T, composed on the host in fp64: fp32 roundings never pile up.
* Matching (cloud_compare, unchanged).  A stage builds CloudGrid(border, h_s) and prepares the reference once.  Each iteration
  prepares P' and calls cloud_compare.nearest(P', Q, grid, ...), which returns e and idx.  A pair counts when idx >= 0 and
  e <= e_max; e_max is 1024 without max_pair_dist, else the bin above.
* Sums (d3d_cloud_register_sums).  The origin is o = (xmin, ymin, zmin) of the border.  Per counted pair
  a_c = llrint(((double)p'_c - o_c) / h * 1024.0), and b_c likewise from Q[idx].  A keyed point lies inside the grid and the grid
  has at most 2^21 - 1 cells per axis, so 0 <= a_c, b_c < 2^31 and every product a_r b_c < 2^62.  sums is int64 [27], zeroed by the
  call:
    [0] N, the counted pairs;  [1..3] sum a;  [4..6] sum b;  [7..15] sum (a_r b_c) & 0xFFFFFFFF, row-major;
    [16..24] sum (a_r b_c) >> 32;  [25] sum e;  [26] sum e^2.
  - With at most 2^31 - 1 points no slot can overflow.  The host recombines M_rc = hi * 2^32 + lo in Python integers.  A plain
    64-bit sum of the products would wrap at four points in the far corner of a large grid: the split is the point of the layout.
  - Integer atomicAdd only: the sums are the same bits for any order of P.
  - They are also the same for any order of Q, PROVIDED no counted query has two nearest reference points at exactly equal distance
    and different positions: the nearest rule then picks the lowest input index, so idx and the sums follow Q's order.  Duplicates
    of one position do not matter.
* Solve (host, fp64; solve() needs no GPU).  H_rc = N M_rc - Sa_r Sb_c as exact Python integers, divided by N^2 in float only
  afterwards.  U, S, Vt = numpy.linalg.svd(H);  R = V diag(1, 1, sign(det(V U^T))) U^T.  The means are o + (h / 1024) S / N;
  t = mean_b - R mean_a.  N < 3 or S[1] <= 1e-12 S[0] ends the stage with the reason "degenerate" and leaves T unchanged;
  otherwise T <- dT @ T.
* Stop.  moved is the largest displacement of the eight corners of the border under dT.  A stage ends when moved < tolerance
  ("converged") or after max_iterations ("iterations").  The next stage starts from the T reached.  One host read per iteration
  (the 27 sums) and one 12-double upload; nothing else crosses the bus.
* Output.  T, a 4 x 4 float64 numpy array; a log with one dict per iteration -- stage, cap, iteration (both counted from 1),
  pairs = N, rms = sqrt(sums[26] / N) / 1024 * h, moved, and on a stage's last entry reason --; P transformed by the final T, on
  the device.

Out of scope: scale (similarity transforms); point-to-plane with reference normals; subsampling; weights; robust kernels beyond the
pair cap; a global, feature-based initial alignment; the shift of large coordinates before the fp32 rounding.  Ground truth is not
an input of a reconstruction run: pipeline.predict_and_fuse and predict have no key or flag for this.  mesh_compare has no
registration of its own: register the mesh's samples (mesh_compare --out_samples) here, then pass the transform to it.

The transform and the sums are HIP (csrc/cloud_register.hip); the keys, the sort and the search are cloud_compare's, as they are.

    python -m deep3d_aerial_amd.cloud_register --cloud A.ply --reference B.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax
        --max_dist H1[,H2...] [--max_pair_dist D] [--iterations K] [--tolerance T] [--init T0.txt] [--out_transform T.txt]
        [--out A_registered.ply] [--json LOG.json]
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import _geom, _lib, cloud, cloud_compare
from ._geom import ptr as _ptr, stream as _stream

CAP = cloud_compare.CAP
SUMS = 27


_VERB = "the clouds are registered"


def _points(xyz, name):
    """xyz checked by name as a cloud on a GPU, contiguous."""
    return cloud.on_gpu(cloud.points(xyz, name), name, _VERB)


# ----------------------------------------------------------------------------------------
# the transform
# ----------------------------------------------------------------------------------------
def _transform(T, name="T"):
    """T as a 4 x 4 float64 array: finite, last row 0 0 0 1."""
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    try:
        T = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s must be a 4 x 4 matrix of numbers" % name)
    if T.shape != (4, 4):
        raise ValueError("%s must be a 4 x 4 matrix (got shape %s)" % (name, T.shape))
    if not np.isfinite(T).all():
        raise ValueError("%s must be finite" % name)
    if T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError("the last row of %s must be 0 0 0 1 (got %s)" % (name, " ".join(repr(v) for v in T[3].tolist())))
    return T


def apply(xyz, T):
    """xyz [n,3] fp32 on one GPU, T a 4 x 4 fp64 matrix whose last row is 0 0 0 1 -> xyz transformed by T as the module's docstring
    states it: a new device tensor queued on the caller's stream.  The host uploads the 12 doubles and reads nothing.  CPU tensors
    are refused."""
    T = _transform(T)
    xyz = _points(xyz, "xyz")
    n, dev = int(xyz.shape[0]), xyz.device
    rt =torch.tensor(T[:3].reshape(-1).tolist(), dtype=torch.float64, device=dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().d3d_cloud_transform(_ptr(xyz) if n else None, n, _ptr(rt), _ptr(out) if n else None, _stream()),
               "d3d_cloud_transform")
    return out


# ----------------------------------------------------------------------------------------
# the sums
# ----------------------------------------------------------------------------------------
def _e_max(e_max):
    if not _geom.is_int(e_max, 0, CAP):
        raise ValueError("e_max must be an integer in 0 .. 1024 (got %r)" % (e_max,))
    return int(e_max)


def pair_sums(moved_xyz, e, idx, reference_xyz, grid, e_max=CAP):
    """moved_xyz [n,3] fp32, e [n] int32 and idx [n] int32 of cloud_compare.nearest(moved_xyz, reference_xyz, grid), reference_xyz
    [m,3] fp32, all on one GPU -> sums [27] int64 of the module's docstring: a device tensor queued on the caller's stream; the host
    reads nothing.  CPU tensors are refused."""
    cloud.check_grid(grid)
    e_max = _e_max(e_max)
    moved_xyz, reference_xyz = cloud.points(moved_xyz, "moved_xyz"), cloud.points(reference_xyz, "reference_xyz")
    n, m = int(moved_xyz.shape[0]), int(reference_xyz.shape[0])
    for t, name in ((e, "e"), (idx, "idx")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise ValueError("%s must be a [%d] int32 tensor (got %s %s)" % (name, n, t.dtype, tuple(t.shape)))
    moved_xyz, reference_xyz = cloud.on_gpu(moved_xyz, "moved_xyz", _VERB), cloud.on_gpu(reference_xyz, "reference_xyz", _VERB)
    dev = moved_xyz.device
    for t, name in ((e, "e"), (idx, "idx"), (reference_xyz, "reference_xyz")):
        if t.device != dev:
            raise RuntimeError("%s is on %s and moved_xyz on %s: the sums are taken on one GPU (no CPU fallback)" % (name, t.device, dev))
    e, idx = e.contiguous(), idx.contiguous()
    sums = torch.empty((SUMS,), dtype=torch.int64, device=dev)   # zeroed by the call
    pn = (lambda t: _ptr(t) if n else None)
    b = grid.border
    _lib.check(_lib.load().d3d_cloud_register_sums(pn(moved_xyz), pn(e), pn(idx), n, _ptr(reference_xyz) if m else None, m, b[0], b[2], b[4],
                                                   grid.voxel, e_max, _ptr(sums), _stream()), "d3d_cloud_register_sums")
    return sums


# ----------------------------------------------------------------------------------------
# the solve (host only)
# ----------------------------------------------------------------------------------------
def _sums(sums):
    if isinstance(sums, torch.Tensor):
        sums = sums.tolist()
    s = [int(v) for v in sums]
    if len(s) != SUMS:
        raise ValueError("sums must hold %d integers (got %d)" % (SUMS, len(s)))
    return s


def solve(sums, grid):
    """The closed-form rigid alignment of the module's docstring from the 27 sums (a list, array or tensor) on `grid`.  Host only, no
    GPU needed.  -> (dT, info): dT a 4 x 4 float64 array that moves the a's onto the b's in the least-squares sense, or None when
    the pairs do not determine one; info = {"pairs": N, "rms": sqrt(sums[26] / N) / 1024 * h (0.0 for N = 0), "degenerate": bool}."""
    cloud.check_grid(grid)
    s = _sums(sums)
    h, N = grid.voxel, s[0]
    if N < 0:
        raise ValueError("sums[0] = %d pairs" % N)
    info = {"pairs": N, "rms": math.sqrt(s[26] / N) / CAP * h if N > 0 else 0.0, "degenerate": True}
    if N < 3:
        return None, info
    Sa, Sb = s[1:4], s[4:7]
    M = [[(s[16 + 3 * r + c] << 32) + s[7 + 3 * r + c] for c in range(3)] for r in range(3)]
    NN = N * N
    H = np.array([[(N * M[r][c] - Sa[r] * Sb[c]) / NN for c in range(3)] for r in range(3)], dtype=np.float64)   # in bins^2
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > 1e-12 * S[0]:
        return None, info
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0.0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    o = np.array(grid.border[0::2], dtype=np.float64)
    mean_a = o + (h / CAP) * np.array([v / N for v in Sa], dtype=np.float64)
    mean_b = o + (h / CAP) * np.array([v / N for v in Sb], dtype=np.float64)
    dT = np.eye(4, dtype=np.float64)
    dT[:3, :3] = R
    dT[:3, 3] = mean_b - R @ mean_a
    info["degenerate"] = False
    return dT, info


def corner_motion(dT, border):
    """The largest displacement of the eight corners of the border under dT (world units)."""
    b = [float(v) for v in border]
    c = np.array([[b[i], b[2 + j], b[4 + k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
    d = c @ dT[:3, :3].T + dT[:3, 3] - c
    return float(np.sqrt((d * d).sum(1)).max())


# ----------------------------------------------------------------------------------------
# the iteration
# ----------------------------------------------------------------------------------------
def _schedule(max_dists):
    try:
        caps = list(max_dists)
    except TypeError:
        caps = [max_dists]
    if not caps:
        raise ValueError("at least one max_dist is needed")
    caps = [cloud_compare.check_max_dist(h) for h in caps]
    if any(b >= a for a, b in zip(caps, caps[1:])):
        raise ValueError("the max_dist schedule must decrease strictly, coarse to fine (got %r)" % (caps,))
    return caps


def _plan(border, max_dists, max_iterations, tolerance, max_pair_dist):
    """[(grid, e_max, tolerance)] per stage, every setting checked."""
    caps = _schedule(max_dists)
    if not _geom.is_int(max_iterations, 1):
        raise ValueError("max_iterations must be an integer >= 1 (got %r)" % (max_iterations,))
    if tolerance is not None and not _geom.is_real(tolerance, above=0):
        raise ValueError("tolerance must be finite and > 0 (got %r)" % (tolerance,))
    stages = []
    for h in caps:
        try:
            grid = cloud.CloudGrid(border, h)
        except ValueError as e:
            raise ValueError("register grid (border, max_dist %r as the voxel): %s" % (h, e))
        try:
            e_max = CAP if max_pair_dist is None else cloud_compare.threshold_bin(max_pair_dist, h)
        except ValueError as e:
            raise ValueError("max_pair_dist: %s" % e)
        stages.append((grid, e_max, float(tolerance) if tolerance is not None else h / CAP))
    return stages


def register(cloud_xyz, reference_xyz, border, max_dists, init=None, max_iterations=50, tolerance=None, max_pair_dist=None):
    """(T, log, moved_xyz): the registration of the module's docstring of the cloud [n,3] fp32 to the reference [m,3] fp32 (device
    tensors on one GPU): T a 4 x 4 float64 numpy array, the log with one dict per iteration, and the cloud transformed by T (a
    device tensor).  The host reads the 27 sums once per iteration.  CPU tensors are refused."""
    stages = _plan(border, max_dists, max_iterations, tolerance, max_pair_dist)
    T = _transform(np.eye(4) if init is None else init, "init")
    cloud_xyz, reference_xyz = _points(cloud_xyz, "cloud_xyz"), _points(reference_xyz, "reference_xyz")
    if cloud_xyz.device != reference_xyz.device:
        raise ValueError("cloud_xyz is on %s and reference_xyz on %s: both clouds must be on one GPU" % (cloud_xyz.device, reference_xyz.device))
    log = []
    for stage, (grid, e_max, tol) in enumerate(stages, 1):
        prepared = cloud_compare.prepare(reference_xyz, grid)
        for iteration in range(1, int(max_iterations) + 1):
            moved_xyz = apply(cloud_xyz, T)
            e, idx, _ = cloud_compare.nearest(moved_xyz, reference_xyz, grid, None, prepared)
            sums = pair_sums(moved_xyz, e, idx, reference_xyz, grid, e_max).tolist()   # the one read
            dT, info = solve(sums, grid)
            entry = {"stage": stage, "cap": grid.voxel, "iteration": iteration, "pairs": info["pairs"], "rms": info["rms"], "moved": 0.0}
            log.append(entry)
            if dT is None:
                entry["reason"] = "degenerate"
                break
            T = dT @ T   # (both last rows are 0 0 0 1, and so is the product's, exactly)
            entry["moved"] = corner_motion(dT, grid.border)
            if entry["moved"] < tol:
                entry["reason"] = "converged"
                break
            if iteration == max_iterations:
                entry["reason"] = "iterations"
    return T, log, apply(cloud_xyz, T)


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def write_transform(path, T):
    """Four lines of four numbers, written with repr: read_transform gives the same bits back."""
    T = _transform(T)
    text = "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in T.tolist())
    _geom.write_bytes(path, text.encode("ascii"))
    return str(path)


def read_transform(path):
    """The 4 x 4 float64 matrix of a file of four lines of four numbers; its last row must be 0 0 0 1 and every number finite."""
    with open(str(path)) as f:
        lines = [ln.split() for ln in f.read().split("\n") if ln.strip()]
    if len(lines) != 4 or any(len(w) != 4 for w in lines):
        raise ValueError("%s: a transform is four lines of four numbers" % path)
    try:
        T = [[float(v) for v in w] for w in lines]
    except ValueError:
        raise ValueError("%s: a transform is four lines of four numbers" % path)
    return _transform(T, str(path))


def xyz_ply_bytes(xyz):
    """The bytes of a binary little-endian PLY with x y z float per point, in input order.  A host array or a tensor."""
    xyz = _geom.host(xyz)
    n = int(xyz.shape[0])
    if xyz.dtype != np.float32 or xyz.shape != (n, 3):
        raise ValueError("xyz must be [n,3] float32 (got %s %s)" % (xyz.shape, xyz.dtype))
    rec = np.ascontiguousarray(xyz, "<f4").view([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]).reshape(n)
    return _geom.record_ply_bytes("registered cloud (deep3d_aerial_amd.cloud_register)", rec)


# ----------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------
def _parse_caps(text):
    try:
        vals = [float(v) for v in str(text).split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("--max_dist needs H1[,H2...] (got %r)" % (text,))
    return vals


def add_transform_argument(ap):
    """--transform of the two compare tools."""
    ap.add_argument("--transform", default=None, help="move the evaluated cloud by this 4 x 4 transform first (.txt of cloud_register)")


def check_transform_argument(ap, path, inputs, outs):
    """The refusals of --transform that need no file read: through ap.error."""
    if path is None:
        return
    if not str(path).endswith(".txt"):
        ap.error("--transform must end in .txt")
    p = os.path.abspath(str(path))
    if p in outs:
        ap.error("an output would overwrite --transform")
    if p in inputs:
        ap.error("--transform names an input cloud")


def main(argv=None):
    ap = argparse.ArgumentParser(description="rigid registration (ICP) of a point cloud to a reference cloud")
    ap.add_argument("--cloud", default=None, help="the evaluated cloud (.ply, binary little-endian)")
    ap.add_argument("--reference", default=None, help="the reference cloud, or a mesh whose vertices serve (.ply)")
    ap.add_argument("--border", type=cloud.parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--max_dist", type=_parse_caps, default=None, help="H1[,H2...]: the cap of the search per stage, decreasing (world units)")
    ap.add_argument("--max_pair_dist", type=float, default=None, help="only pairs within this distance count (world units)")
    ap.add_argument("--iterations", type=int, default=50, help="iterations per stage at most")
    ap.add_argument("--tolerance", type=float, default=None, help="a stage ends when the border's corners move less (default: max_dist / 1024)")
    ap.add_argument("--init", default=None, help="the initial transform (.txt: four lines of four numbers)")
    ap.add_argument("--out_transform", default=None, help="write the transform here (.txt)")
    ap.add_argument("--out", default=None, help="write the registered cloud here (.ply)")
    ap.add_argument("--json", default=None, help="write the result here too (.json)")
    a = ap.parse_args(argv)
    for flag in ("cloud", "reference", "border", "max_dist"):
        if getattr(a, flag) is None:
            ap.error("--%s is required" % flag)
    for flag, end in (("init", ".txt"), ("out_transform", ".txt"), ("out", ".ply"), ("json", ".json")):
        if getattr(a, flag) is not None and not str(getattr(a, flag)).endswith(end):
            ap.error("--%s must end in %s" % (flag, end))
    outs = [os.path.abspath(str(p)) for p in (a.out_transform, a.out, a.json) if p is not None]   # (three endings: no two can agree)
    inputs = {os.path.abspath(str(p)) for p in (a.cloud, a.reference, a.init) if p is not None}
    if set(outs) & inputs:
        ap.error("an output would overwrite an input")
    try:
        _plan(a.border, a.max_dist, a.iterations, a.tolerance, a.max_pair_dist)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the clouds are registered on the GPU (no CPU fallback)")
    init = read_transform(a.init) if a.init is not None else None
    xa, xb = cloud_compare.read_xyz_ply(a.cloud), cloud_compare.read_xyz_ply(a.reference)
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    T, log, moved = register(da, db, a.border, a.max_dist, init, a.iterations, a.tolerance, a.max_pair_dist)
    result = {"transform": T.tolist(), "iterations": len(log), "stages": [e for e in log if "reason" in e], "log": log}
    line = json.dumps(result)
    if a.out_transform is not None:
        write_transform(a.out_transform, T)
    if a.out is not None:
        _geom.write_bytes(a.out, xyz_ply_bytes(moved))
    if a.json is not None:
        _geom.write_bytes(a.json, (line + "\n").encode("ascii"))
    print(line)
    return result


if __name__ == "__main__":
    main()
