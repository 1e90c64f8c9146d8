"""The numpy restatement of the normals of a point cloud (deep3d_aerial_amd/cloud_normals.py, csrc/cloud_normals.hip, DESIGN.md
§4.34) and the scene its tests share.  `sums_numpy` is the ten integer sums over all pairs, O(n^2); `normals_numpy` is everything
after them with numpy.linalg.eigh in place of the device's Jacobi sweeps: the sums must agree bit for bit, the normals in angle.

The rule: on CloudGrid(border, h) a keyed point i has as neighbours the keyed points j, itself included, of the 27 cells around its
cell with d2 = (dx dx + dy dy) + dz dz < h h in fp64.  Per neighbour delta_c = rint(((double)x_jc - (double)x_ic) / h * 1024.0).
Sums: k, S1[3] = sum delta, S2[6] = sum delta_r delta_c (xx xy xz yy yz zz).  C_rc = S2_rc - (S1_r * S1_c) / k in fp64.  l0 <= l1 <=
l2 and the unit eigenvector n of l0, flipped so that n . up >= 0 (up = +z, or -z with z_down; where n . up == 0 the first non-zero
component positive).  flatness = rint(1024 l0 / (l0 + l1 + l2)).  Degenerate (k < 3, l2 <= 0 or l1 <= 1e-12 l2): zero normal,
flatness -1.  An unkeyed point: count 0."""
import functools

import numpy as np

import cloud_register_scene as CRS
import test_cloud as TC
from deep3d_aerial_amd import cloud

BORDER = CRS.BORDER
RADIUS = 3.0          # about three spacings of the 700-point scene: some 25 neighbours a point
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def sums_numpy(xyz, grid):
    """[n,10] int64: k, S1 x y z, S2 xx xy xz yy yz zz of every point; zeros for an unkeyed one."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok, cell, _ = TC.cells_numpy(x, grid)
    X, h = x.astype(np.float64), np.float64(grid.voxel)
    out = np.zeros((len(x), 10), np.int64)
    for i in np.nonzero(ok)[0]:
        with np.errstate(invalid="ignore", over="ignore"):
            d = X[i] - X
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            near = ok & (np.abs(cell - cell[i]) <= 1).all(1) & (d2 < h * h)
        delta = np.rint((X[near] - X[i]) / h * 1024.0).astype(np.int64)
        out[i, 0] = len(delta)
        out[i, 1:4] = delta.sum(0)
        out[i, 4:] = [(delta[:, r] * delta[:, c]).sum() for r, c in PAIRS]
    return out


def covariance_numpy(s):
    """C [3,3] float64 of one row of the sums with k > 0, each operation rounded once."""
    k, S1 = np.float64(s[0]), s[1:4].astype(np.float64)
    C = np.zeros((3, 3))
    for v, (r, c) in zip(s[4:].astype(np.float64), PAIRS):
        C[r, c] = C[c, r] = v - (S1[r] * S1[c]) / k
    return C


def normals_numpy(sums, z_down=False):
    """(normal [n,3] float64, count [n], flatness [n], well [n] bool) from the sums: well marks the points whose two smallest
    eigenvalues are apart by more than 1e-3 of the largest, where eigh's eigenvector is itself well defined."""
    n = len(sums)
    normal, flat, well = np.zeros((n, 3)), np.full(n, -1, np.int64), np.zeros(n, bool)
    up = -1.0 if z_down else 1.0
    for i, s in enumerate(sums):
        if s[0] < 3:
            continue
        lam, V = np.linalg.eigh(covariance_numpy(s))
        if not (lam[2] > 0.0 and lam[1] > 1e-12 * lam[2]):
            continue
        v = V[:, 0] / np.sqrt(V[:, 0] @ V[:, 0])
        d = v[2] * up
        if d < 0 or (d == 0 and (v[0] < 0 or (v[0] == 0 and v[1] < 0))):
            v = -v
        normal[i], flat[i] = v, int(np.rint(1024.0 * lam[0] / (lam[0] + lam[1] + lam[2])))
        well[i] = lam[1] - lam[0] > 1e-3 * lam[2]
    return normal, sums[:, 0].copy(), flat, well


def angle(a, b):
    """The angle between the lines of a and b [n,3], in radians, fp64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(1)), np.abs((a * b).sum(1)))


def grid():
    return cloud.CloudGrid(BORDER, RADIUS)


@functools.lru_cache(maxsize=None)
def scene():
    """(xyz [n,3] float32, parts): 700 points of the registration scene's surface and, appended in this order, parts = {name:
    slice}: "duplicates" 40 copies of one surface point (a range longer than the walk's look-ahead); "corners" four points in each
    of the grid's two corner cells (clipped windows); "apart" two points exactly one radius apart and further than that from
    everything else (each other's non-neighbour: count 1); "unkeyed" two points outside the border and a NaN.  Callers do not
    change what they get."""
    rng = np.random.default_rng(5)
    base = CRS.surface(3, 700).astype(np.float32)
    pieces = {"duplicates": np.repeat(base[17:18], 40, 0),
              "corners": np.concatenate([rng.uniform(0.05, 0.9, (4, 3)), np.array([32.0, 32.0, 16.0]) - rng.uniform(0.05, 0.9, (4, 3))]),
              "apart": np.array([[30.0, 1.0, 14.5], [27.0, 1.0, 14.5]]),
              "unkeyed": np.array([[-0.5, 3.0, 3.0], [5.0, 5.0, 18.5], [np.nan, 1.0, 1.0]])}
    parts, at, out = {"surface": slice(0, 700)}, 700, [base]
    for name, p in pieces.items():
        parts[name] = slice(at, at + len(p))
        at += len(p)
        out.append(p.astype(np.float32))
    xyz = np.concatenate(out)
    xyz.setflags(write=False)
    return xyz, parts


@functools.lru_cache(maxsize=None)
def expected(z_down=False):
    """(sums, normal, count, flatness, well) of the scene, computed once and shared."""
    s = sums_numpy(scene()[0], grid())
    out = (s,) + normals_numpy(s, z_down)
    for a in out:
        a.setflags(write=False)
    return out
