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

* Point-to-plane (metric="plane").  Against a discrete sample of a surface the sums above pull every point to
  the nearest SAMPLE, and the residual stops at a fraction of the reference's spacing.  With the reference's normals -- given,
  or estimated once by cloud_normals.estimate(Q, border, normal_radius, z_down) -- the step minimises the distance to the
  reference's tangent planes instead.  The matching and the loop are the ones above; the sums and the solve are these.
  - Sums (d3d_cloud_register_plane_sums).  a, b are the bins above; c_c = 512 n_c is the grid's centre in the same units;
    m_c = llrint((double)normal_c * 1024.0) of the matched reference point.  A pair counts when it counts above and its normal is
    finite with every |normal_c| <= 1 and m != (0, 0, 0).  Per counted pair u = a - c, r = (a - b) . m, w = u x m and
    g = (w_x, w_y, w_z, m_x, m_y, m_z): the residual linearised under a rotation omega about c and a translation tau (in bins)
    is r + g . (omega, tau).  sums is int64 [87], zeroed by the call: [0] N, [1] sum e, [2] sum e^2, then 28 products P_k -- the 21
    g_i g_j, i <= j, row-major; the 6 g_i r; r r --, each a 128-bit two's-complement value summed in three slots 3 + 3k .. 5 + 3k:
    the low 32 bits of its low word, the high 32 bits of its low word (both unsigned) and its signed high word: the hi / lo split
    above with one more limb, for the same reason.  |w| < 2^42, |r| < 2^43, |P| < 2^87, and 2^31 - 1 pairs overflow no slot.
    Integer atomicAdd only: the same bits for any order of P.
  - Solve (solve_plane, host, fp64).  H = sum g g^T (6 x 6) and v = sum g r recombined exactly in Python integers.  With
    D = sqrt(diag H), Hn = H / (D D^T) and vn = v / D; an unknown whose diagonal is zero is dropped.  lam, Q = numpy.linalg.eigh(Hn);
    the directions with lam < min_eig_ratio (1e-6) times the largest are dropped: the sums are exact, so only the geometry limits
    the conditioning, and a flat scene leaves its in-plane motion where it is.  xi = -D^-1 Q diag(1 / lam) Q^T vn = (omega, tau).
    dT rotates by the exact Rodrigues matrix of omega about the world point of c and translates by tau h / 1024.  N < 6 or no
    direction kept is "degenerate".  The log entries gain plane_rms = sqrt(sum r r / N) / 1024^2 h and rank.

Out of scope: scale (similarity transforms); subsampling; weights; robust kernels beyond the
pair cap; a global, feature-based initial alignment; the shift of large coordinates before the fp32 rounding.  Ground truth is not
an input of a reconstruction run: pipeline.predict_and_fuse and predict have no key or flag for this.  mesh_compare has no
registration of its own: register the mesh's samples (mesh_compare --out_samples) here, then pass the transform to it.

The transform and the sums are HIP (csrc/cloud_register.hip); the keys, the sort and the search are cloud_compare's, as they are.

    python -m deep3d_aerial_amd.cloud_register --cloud A.ply --reference B.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax
        --max_dist H1[,H2...] [--max_pair_dist D] [--iterations K] [--tolerance T] [--init T0.txt] [--out_transform T.txt]
        [--out A_registered.ply] [--json LOG.json] [--metric point|plane] [--normal_radius R] [--z_down]
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
PLANE_SUMS = 87
METRICS = ("point", "plane")


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


def _pairs(moved_xyz, e, idx, reference_xyz, reference_normals=None):
    """The arguments of the two sums checked and contiguous on one GPU: (moved_xyz, e, idx, reference_xyz, reference_normals)."""
    moved_xyz, reference_xyz = cloud.points(moved_xyz, "moved_xyz"), cloud.points(reference_xyz, "reference_xyz")
    n, m = int(moved_xyz.shape[0]), int(reference_xyz.shape[0])
    for t, name in ((e, "e"), (idx, "idx")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise ValueError("%s must be a [%d] int32 tensor (got %s %s)" % (name, n, t.dtype, tuple(t.shape)))
    if reference_normals is not None and int(cloud.points(reference_normals, "reference_normals").shape[0]) != m:
        raise ValueError("reference_xyz has %d points, reference_normals %d" % (m, reference_normals.shape[0]))
    moved_xyz, reference_xyz = cloud.on_gpu(moved_xyz, "moved_xyz", _VERB), cloud.on_gpu(reference_xyz, "reference_xyz", _VERB)
    if reference_normals is not None:
        reference_normals = cloud.on_gpu(reference_normals, "reference_normals", _VERB)
    dev = moved_xyz.device
    for t, name in ((e, "e"), (idx, "idx"), (reference_xyz, "reference_xyz"), (reference_normals, "reference_normals")):
        if t is not None and t.device != dev:
            raise RuntimeError("%s is on %s and moved_xyz on %s: the sums are taken on one GPU (no CPU fallback)" % (name, t.device, dev))
    return moved_xyz, e.contiguous(), idx.contiguous(), reference_xyz, reference_normals


def pair_sums(moved_xyz, e, idx, reference_xyz, grid, e_max=CAP):
    """moved_xyz [n,3] fp32, e [n] int32 and idx [n] int32 of cloud_compare.nearest(moved_xyz, reference_xyz, grid), reference_xyz
    [m,3] fp32, all on one GPU -> sums [27] int64 of the module's docstring: a device tensor queued on the caller's stream; the host
    reads nothing.  CPU tensors are refused."""
    cloud.check_grid(grid)
    e_max = _e_max(e_max)
    moved_xyz, e, idx, reference_xyz, _ = _pairs(moved_xyz, e, idx, reference_xyz)
    n, m, dev = int(moved_xyz.shape[0]), int(reference_xyz.shape[0]), moved_xyz.device
    sums = torch.empty((SUMS,), dtype=torch.int64, device=dev)   # zeroed by the call
    pn = (lambda t: _ptr(t) if n else None)
    b = grid.border
    _lib.check(_lib.load().d3d_cloud_register_sums(pn(moved_xyz), pn(e), pn(idx), n, _ptr(reference_xyz) if m else None, m, b[0], b[2], b[4],
                                                   grid.voxel, e_max, _ptr(sums), _stream()), "d3d_cloud_register_sums")
    return sums


def plane_sums(moved_xyz, e, idx, reference_xyz, reference_normals, grid, e_max=CAP):
    """pair_sums' inputs and reference_normals [m,3] fp32 -> sums [87] int64 of the point-to-plane metric (the module's docstring):
    a device tensor queued on the caller's stream; the host reads nothing.  CPU tensors are refused."""
    cloud.check_grid(grid)
    e_max = _e_max(e_max)
    if reference_normals is None:
        raise ValueError("the plane sums need reference_normals")
    moved_xyz, e, idx, reference_xyz, reference_normals = _pairs(moved_xyz, e, idx, reference_xyz, reference_normals)
    n, m, dev = int(moved_xyz.shape[0]), int(reference_xyz.shape[0]), moved_xyz.device
    sums = torch.empty((PLANE_SUMS,), dtype=torch.int64, device=dev)   # zeroed by the call
    pn, pm = (lambda t: _ptr(t) if n else None), (lambda t: _ptr(t) if m else None)
    b = grid.border
    _lib.check(_lib.load().d3d_cloud_register_plane_sums(pn(moved_xyz), pn(e), pn(idx), n, pm(reference_xyz), pm(reference_normals), m,
                                                         grid.n[0], grid.n[1], grid.n[2], b[0], b[2], b[4], grid.voxel, e_max, _ptr(sums),
                                                         _stream()), "d3d_cloud_register_plane_sums")
    return sums


# ----------------------------------------------------------------------------------------
# the solve (host only)
# ----------------------------------------------------------------------------------------
def _sums(sums, count=None):
    count = SUMS if count is None else count
    if isinstance(sums, torch.Tensor):
        sums = sums.tolist()
    s = [int(v) for v in sums]
    if len(s) != count:
        raise ValueError("sums must hold %d integers (got %d)" % (count, len(s)))
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


def plane_products(sums):
    """The 28 products of the 87 plane sums recombined in Python integers, hi 2^64 + mid 2^32 + lo each:
    (H, v, rr): H the 6 x 6 symmetric sum of g g^T, v the sum of g r (6), rr the sum of r r."""
    s = _sums(sums, PLANE_SUMS)
    P = [(s[5 + 3 * k] << 64) + (s[4 + 3 * k] << 32) + s[3 + 3 * k] for k in range(28)]
    H = [[0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = P[k]
            k += 1
    return H, P[21:27], P[27]


def solve_plane(sums, grid, min_eig_ratio=1e-6):
    """The point-to-plane step of the module's docstring from the 87 sums (a list, array or tensor) on `grid`.  Host only, no GPU
    needed.  -> (dT, info): dT a 4 x 4 float64 array, or None when the pairs do not determine one; info = {"pairs": N, "rms":
    sqrt(sums[2] / N) / 1024 * h, "plane_rms": sqrt(sum r r / N) / 1024^2 * h (both 0.0 for N = 0), "rank": the directions kept,
    "degenerate": N < 6 or rank 0}."""
    cloud.check_grid(grid)
    if not (_geom.is_real(min_eig_ratio, above=0) and min_eig_ratio < 1):
        raise ValueError("min_eig_ratio must lie in (0, 1) (got %r)" % (min_eig_ratio,))
    s = _sums(sums, PLANE_SUMS)
    H, v, rr = plane_products(s)
    h, N = grid.voxel, s[0]
    if N < 0 or rr < 0:
        raise ValueError("plane sums of %d pairs, sum r r = %d" % (N, rr))
    info = {"pairs": N, "rms": math.sqrt(s[2] / N) / CAP * h if N > 0 else 0.0,
            "plane_rms": math.sqrt(rr / N) / (CAP * CAP) * h if N > 0 else 0.0, "rank": 0, "degenerate": True}
    if N < 6:
        return None, info
    D = [math.sqrt(H[i][i]) for i in range(6)]   # (a sum of squares: >= 0)
    live = [i for i in range(6) if D[i] > 0.0]   # a zero diagonal: no pair constrains that unknown
    if not live:
        return None, info
    Hn = np.array([[H[i][j] / (D[i] * D[j]) for j in live] for i in live], dtype=np.float64)
    vn = np.array([v[i] / D[i] for i in live], dtype=np.float64)
    lam, Q = np.linalg.eigh(Hn)
    keep = lam >= float(min_eig_ratio) * lam[-1]
    keep &= lam > 0.0
    info["rank"] = int(keep.sum())
    if info["rank"] == 0:
        return None, info
    Qk = Q[:, keep]
    xn = -(Qk @ ((Qk.T @ vn) / lam[keep]))
    xi = np.zeros(6, dtype=np.float64)
    xi[live] = xn / np.array([D[i] for i in live], dtype=np.float64)
    omega, tau = xi[:3], xi[3:]   # radians about c, bins
    theta = float(np.sqrt(omega @ omega))
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if theta > 0.0:   # Rodrigues: R = I + sin(theta) / theta K + (1 - cos(theta)) / theta^2 K K, 1 - cos as 2 sin^2 of the half
        R = np.eye(3) + (math.sin(theta) / theta) * K + (2.0 * math.sin(0.5 * theta) ** 2 / (theta * theta)) * (K @ K)
    else:
        R = np.eye(3)
    c = np.array([grid.border[2 * a] + 0.5 * grid.n[a] * h for a in range(3)], dtype=np.float64)   # the world point of c = 512 n
    dT = np.eye(4, dtype=np.float64)
    dT[:3, :3] = R
    dT[:3, 3] = (c - R @ c) + tau * (h / CAP)
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


def check_metric(metric, reference_normals=None, normal_radius=None, border=None):
    """The metric's settings checked without GPU work: "point" takes neither normals nor a radius; "plane" needs exactly one."""
    if metric not in METRICS:
        raise ValueError("metric must be one of %s (got %r)" % (", ".join(METRICS), metric))
    if metric == "point":
        if reference_normals is not None or normal_radius is not None:
            raise ValueError("reference_normals and normal_radius belong to metric=\"plane\"")
        return
    if (reference_normals is None) == (normal_radius is None):
        raise ValueError("metric=\"plane\" needs reference_normals or a normal_radius, one of the two")
    if normal_radius is not None:
        try:
            cloud.CloudGrid(border, normal_radius)
        except ValueError as e:
            raise ValueError("normals grid (border, normal_radius as the voxel): %s" % e)


def register(cloud_xyz, reference_xyz, border, max_dists, init=None, max_iterations=50, tolerance=None, max_pair_dist=None,
             metric="point", reference_normals=None, normal_radius=None, z_down=False):
    """(T, log, moved_xyz): the registration of the module's docstring of the cloud [n,3] fp32 to the reference [m,3] fp32 (device
    tensors on one GPU): T a 4 x 4 float64 numpy array, the log with one dict per iteration, and the cloud transformed by T (a
    device tensor).  The host reads the sums (27, or 87 with metric="plane") once per iteration.  metric="plane" takes the
    reference's normals as reference_normals [m,3] fp32, or estimates them once with cloud_normals.estimate(reference_xyz, border,
    normal_radius, z_down).  CPU tensors are refused."""
    stages = _plan(border, max_dists, max_iterations, tolerance, max_pair_dist)
    check_metric(metric, reference_normals, normal_radius, border)
    T = _transform(np.eye(4) if init is None else init, "init")
    cloud_xyz, reference_xyz = _points(cloud_xyz, "cloud_xyz"), _points(reference_xyz, "reference_xyz")
    if cloud_xyz.device != reference_xyz.device:
        raise ValueError("cloud_xyz is on %s and reference_xyz on %s: both clouds must be on one GPU" % (cloud_xyz.device, reference_xyz.device))
    plane = metric == "plane"
    if plane and reference_normals is None:
        from . import cloud_normals

        reference_normals = cloud_normals.estimate(reference_xyz, border, normal_radius, z_down)[0]
    log = []
    for stage, (grid, e_max, tol) in enumerate(stages, 1):
        prepared = cloud_compare.prepare(reference_xyz, grid)
        for iteration in range(1, int(max_iterations) + 1):
            moved_xyz = apply(cloud_xyz, T)
            e, idx, _ = cloud_compare.nearest(moved_xyz, reference_xyz, grid, None, prepared)
            if plane:
                dT, info = solve_plane(plane_sums(moved_xyz, e, idx, reference_xyz, reference_normals, grid, e_max).tolist(), grid)   # the one read
            else:
                sums = pair_sums(moved_xyz, e, idx, reference_xyz, grid, e_max).tolist()   # the one read
                dT, info = solve(sums, grid)
            entry = {"stage": stage, "cap": grid.voxel, "iteration": iteration, "pairs": info["pairs"], "rms": info["rms"], "moved": 0.0}
            if plane:
                entry["plane_rms"], entry["rank"] = info["plane_rms"], info["rank"]
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
    ap.add_argument("--metric", choices=METRICS, default="point", help="point: to the nearest reference point; plane: to its tangent plane")
    ap.add_argument("--normal_radius", type=float, default=None,
                    help="plane: estimate the reference's normals at this radius (default: the normals the reference file has)")
    ap.add_argument("--z_down", action="store_true", default=False, help="plane: orient the estimated normals towards -Z")
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
    if a.metric == "point" and (a.normal_radius is not None or a.z_down):
        ap.error("--normal_radius and --z_down belong to --metric plane")
    try:
        _plan(a.border, a.max_dist, a.iterations, a.tolerance, a.max_pair_dist)
        if a.normal_radius is not None:
            check_metric(a.metric, None, a.normal_radius, a.border)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the clouds are registered on the GPU (no CPU fallback)")
    init = read_transform(a.init) if a.init is not None else None
    xa, (xb, nb) = cloud_compare.read_xyz_ply(a.cloud), cloud_compare.read_xyz_ply(a.reference, normals=True)
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    normals = None
    if a.metric == "plane" and a.normal_radius is None:
        if nb is None:
            raise ValueError("%s has no nx ny nz: --metric plane needs them or --normal_radius" % a.reference)
        normals = torch.from_numpy(nb).cuda()
    T, log, moved = register(da, db, a.border, a.max_dist, init, a.iterations, a.tolerance, a.max_pair_dist, a.metric, normals,
                             a.normal_radius, a.z_down)
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
