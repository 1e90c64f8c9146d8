"""The numpy restatement of the registration (deep3d_aerial_amd/cloud_register.py, csrc/cloud_register.hip) and the
scenes its tests share.  `transform_numpy` is the transform op by op in fp64, `sums_numpy` the 27 sums in integers that cannot
overflow, `register_numpy` the iteration with the cell-list nearest of tests/test_cloud_compare.py and the module's own solve():
if the kernels' sums are bit-equal to these, everything after them is the same host code."""
import functools
import math

import numpy as np

import test_cloud_compare as TCC
from deep3d_aerial_amd import cloud, cloud_compare as CC, cloud_register as CR

BORDER = [0.0, 32.0, 0.0, 32.0, 0.0, 16.0]
SPACING = 0.5          # about the distance between neighbouring points of the scene: 3000 points on 27.4 x 27.4
N_SCENE = 3000


def transform_numpy(xyz, T):
    """p'_r = (float)(((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]), every operation fp64 and rounded once."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
        return np.stack(rows, 1).astype(np.float32)


def bins_numpy(xyz, grid):
    """a_c = rint(((double)p_c - o_c) / h * 1024.0) per point and axis, int64."""
    o = np.array(grid.border[0::2], np.float64)
    return np.rint((np.asarray(xyz, np.float32).astype(np.float64) - o) / np.float64(grid.voxel) * 1024.0).astype(np.int64)


def sums_numpy(moved, e, idx, reference, grid, e_max=1024):
    """The 27 sums as a list of Python integers.  A pair counts when 0 <= idx < len(reference) and e <= e_max (an idx outside the
    reference is ignored).  Up to 5000 pairs every sum is taken in Python integers; beyond, in int64, where no slot can overflow
    (each split limb is below 2^32 and there are fewer than 2^31 pairs) -- the two routes are checked against each other."""
    moved, reference = np.asarray(moved, np.float32).reshape(-1, 3), np.asarray(reference, np.float32).reshape(-1, 3)
    e, idx = np.asarray(e, np.int64), np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < len(reference)) & (e <= e_max)
    a = bins_numpy(moved[ok], grid)
    b = bins_numpy(reference[idx[ok]], grid)
    ee = e[ok]
    if len(a) <= 5000:
        A, B, E = a.tolist(), b.tolist(), ee.tolist()
        prod = [[[x[r] * y[c] for x, y in zip(A, B)] for c in range(3)] for r in range(3)]
        return ([len(A)] + [sum(x[c] for x in A) for c in range(3)] + [sum(y[c] for y in B) for c in range(3)]
                + [sum(m & 0xFFFFFFFF for m in prod[r][c]) for r in range(3) for c in range(3)]
                + [sum(m >> 32 for m in prod[r][c]) for r in range(3) for c in range(3)] + [sum(E), sum(v * v for v in E)])
    assert a.size == 0 or (a.min() >= 0 and b.min() >= 0 and a.max() < 1 << 31 and b.max() < 1 << 31)
    prod = a[:, :, None] * b[:, None, :]   # below 2^62
    return ([len(a)] + a.sum(0).tolist() + b.sum(0).tolist() + (prod & 0xFFFFFFFF).sum(0).reshape(-1).tolist()
            + (prod >> 32).sum(0).reshape(-1).tolist() + [int(ee.sum()), int((ee * ee).sum())])


def register_numpy(cloud_xyz, reference_xyz, border, max_dists, init=None, max_iterations=50, tolerance=None, max_pair_dist=None):
    """(T, log, moved_xyz) of cloud_register.register, with the restatements above in place of the kernels."""
    P, Q = np.asarray(cloud_xyz, np.float32).reshape(-1, 3), np.asarray(reference_xyz, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    log = []
    for stage, h in enumerate(max_dists, 1):
        grid = cloud.CloudGrid(border, h)
        e_max = 1024 if max_pair_dist is None else CC.threshold_bin(max_pair_dist, h)
        tol = h / 1024 if tolerance is None else tolerance
        for iteration in range(1, max_iterations + 1):
            moved = transform_numpy(P, T)
            e, idx, _ = TCC.nearest_cells(moved, Q, grid)
            dT, info = CR.solve(sums_numpy(moved, e, idx, Q, grid, e_max), grid)
            entry = {"stage": stage, "cap": grid.voxel, "iteration": iteration, "pairs": info["pairs"], "rms": info["rms"], "moved": 0.0}
            log.append(entry)
            if dT is None:
                entry["reason"] = "degenerate"
                break
            T = dT @ T
            entry["moved"] = CR.corner_motion(dT, grid.border)
            if entry["moved"] < tol:
                entry["reason"] = "converged"
                break
            if iteration == max_iterations:
                entry["reason"] = "iterations"
    return T, log, transform_numpy(P, T)


# ----------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------
def height(x, y):
    """A heightfield with two raised blocks."""
    z = 4.0 + 1.5 * np.sin(0.45 * x) * np.cos(0.3 * y) + 0.08 * x
    z = z + 3.0 * ((x > 8) & (x < 14) & (y > 10) & (y < 19))
    return z + 2.0 * ((x > 20) & (x < 25) & (y > 5) & (y < 9))


def surface(seed, n=N_SCENE):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(2.3, 29.7, n), rng.uniform(2.3, 29.7, n)
    return np.stack([x, y, height(x, y)], 1)


def motion():
    """The 4 x 4 fp64 motion of the evaluated cloud: 1.5 degrees about z and 0.75 about x around the border's centre, then a shift
    by (0.25, -0.2, 0.15)."""
    az, ax = math.radians(1.5), math.radians(0.75)
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    c = np.array([16.0, 16.0, 8.0])
    M = np.eye(4)
    M[:3, :3] = Rx @ Rz
    M[:3, 3] = c - M[:3, :3] @ c + np.array([0.25, -0.2, 0.15])
    return M


def scene(separate):
    """(cloud, reference, truth): the reference is a sample of the surface; the evaluated cloud is the same sample (separate =
    False) or a separately drawn one (True), moved by motion(); truth is the transform that takes it back, motion()^-1."""
    M = motion()
    ref = surface(1)
    src = surface(2) if separate else ref
    moved = src @ M[:3, :3].T + M[:3, 3]
    return moved.astype(np.float32), ref.astype(np.float32), np.linalg.inv(M)


def corner_error(T, truth, border=BORDER):
    """The largest distance between the images of the border's eight corners under T and under truth."""
    c = np.array([[border[i], border[2 + j], border[4 + k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    d = (c @ np.asarray(T).T - c @ np.asarray(truth).T)[:, :3]
    return float(np.sqrt((d * d).sum(1)).max())


@functools.lru_cache(maxsize=None)
def registered(separate, caps):
    """register_numpy on scene(separate) with the caps (a tuple), computed once and shared: (T, log, moved).  Callers do not change
    what they get."""
    p, q, _ = scene(separate)
    T, log, moved = register_numpy(p, q, BORDER, list(caps))
    T.setflags(write=False)
    moved.setflags(write=False)
    return T, log, moved
