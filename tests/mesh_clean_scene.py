"""Scenes with floaters for the mesh cleaning tests (tests/test_mesh_clean_gpu.py): ground and the two boxes of
tests/mesh_scene.boxes_scene, plus small boxes hanging in mid-air, ray-cast into the depth map of every view that sees them.
(Wrong depth in a few views only would not do: the TSDF averages those views' negative distances with the free-space votes of
the others, and no surface forms.)  A scene is (grid border, voxel size, [view dicts], FLOATERS, true height function)."""
import numpy as np

import mesh_scene as MS

FLOATERS = [(-5.5, -4.5, 3.0, 4.0, 2.5, 3.25), (4.0, 5.0, -4.5, -3.5, 3.0, 3.75)]   # x0, x1, y0, y1, z0, z1: over open ground


def box_hits(C0, d, lo, hi):
    """Ray parameter of the first hit of the box [lo, hi] (inf: none)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo - C0) / d
        t1 = (hi - C0) / d
    tn = np.nanmax(np.minimum(t0, t1), 1)
    tf = np.nanmin(np.maximum(t0, t1), 1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def floater_scene(seed=4, w=96, h=72, n_views=12, floaters=FLOATERS):
    """Ground z = 0, the boxes of mesh_scene.BOXES and `floaters`, seen from n_views cameras 11-14 m up (no holes)."""
    rng = np.random.default_rng(seed)
    border, voxel = [-7.9, 7.1, -6.0, 6.0, -1.1, 4.3], 0.25
    views = []
    for _ in range(n_views):
        C = (rng.uniform(-5, 5), rng.uniform(-4, 4), rng.uniform(11, 14))
        T = (rng.uniform(-2, 2), rng.uniform(-2, 2), 0.0)
        K = MS.intrinsics(w, h, 0.6 * w)
        E = MS.look_at(C, T)
        C0, d = MS.rays(K, E, w, h)
        lam = np.where(d[:, 2] < 0, -C0[2] / d[:, 2], np.inf)
        for x0, x1, y0, y1, z1 in MS.BOXES:
            lam = np.minimum(lam, box_hits(C0, d, (x0, y0, 0.0), (x1, y1, z1)))
        for x0, x1, y0, y1, z0, z1 in floaters:
            lam = np.minimum(lam, box_hits(C0, d, (x0, y0, z0), (x1, y1, z1)))
        depth, conf = MS._finish(lam, w, h, rng, False)
        views.append({"K": K, "E": E, "depth": depth, "confidence": np.maximum(conf, 0.5).astype(np.float32)})

    def height_near(x, y, r):
        """The highest true surface (ground and boxes, not the floaters) within r of (x, y), per axis."""
        z = np.zeros(np.broadcast(x, y).shape)
        for x0, x1, y0, y1, z1 in MS.BOXES:
            z = np.where((x > x0 - r) & (x < x1 + r) & (y > y0 - r) & (y < y1 + r), np.maximum(z, z1), z)
        return z

    return border, voxel, views, floaters, height_near
