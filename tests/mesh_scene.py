"""Analytic scenes for the mesh (tests/test_mesh.py, tests/test_mesh_gpu.py): numpy ray-cast depth and confidence maps of a
tilted plane, ground with axis-aligned boxes, and a sphere seen from all around.  Maps carry holes (0 and NaN) and low-confidence
pixels; some views reach past the grid, and one camera of the plane scene stands inside the grid, so part of it lies behind it.

A scene is (grid border, voxel size, [view dicts {"K", "E", "depth", "confidence"}], surface distance function)."""
import numpy as np


def look_at(C, target, up=(0.0, 0.0, 1.0)):
    """E = Tcw [4,4] of a camera at C looking at target (x right, y down in the image)."""
    C, target = np.asarray(C, np.float64), np.asarray(target, np.float64)
    f = target - C
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    if np.linalg.norm(r) < 1e-9:
        r = np.cross(f, np.array([0.0, 1.0, 0.0]))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ C
    return E.astype(np.float32)


def intrinsics(w, h, f):
    return np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)


def rays(K, E, w, h):
    """Camera centre [3] and world directions [h*w, 3] whose camera z component is 1 (so the ray parameter is the depth)."""
    K, E = K.astype(np.float64), E.astype(np.float64)
    R, t = E[:3, :3], E[:3, 3]
    ys, xs = np.mgrid[0:h, 0:w]
    dc = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    return -R.T @ t, (R.T @ dc).T


def _finish(lam, w, h, rng, holes):
    lam = np.where(np.isfinite(lam) & (lam > 0), lam, 0.0).reshape(h, w).astype(np.float32)
    conf = rng.uniform(0.3, 1.0, (h, w)).astype(np.float32)
    conf[rng.uniform(size=(h, w)) < 0.05] = rng.uniform(0.0, 0.19)
    if holes:
        lam[rng.uniform(size=(h, w)) < 0.03] = 0.0
        lam[rng.uniform(size=(h, w)) < 0.02] = np.nan
    return lam, conf


def plane_scene(seed=0, w=160, h=120, holes=True):
    """z = 0.1 x - 0.05 y + 2 over a 16 x 16 m grid at 0.25 m; views from 12-15 m up, two reaching past the grid, one standing
    inside the grid and looking along it."""
    rng = np.random.default_rng(seed)
    a, b, c = 0.1, -0.05, 2.0
    border, voxel = [-8.0, 8.0, -8.0, 8.0, -1.0, 5.0], 0.25
    cams = [((rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(12, 15)), (rng.uniform(-2, 2), rng.uniform(-2, 2), 2.0)) for _ in range(6)]
    cams += [((14.0, 0.0, 13.0), (9.0, 0.0, 2.0)), ((-3.0, 12.0, 12.0), (-3.0, 8.0, 2.0)), ((0.0, -6.0, 4.5), (0.0, 6.0, 2.0))]
    views = []
    for C, T in cams:
        K = intrinsics(w, h, 0.8 * w)
        E = look_at(C, T)
        C0, d = rays(K, E, w, h)
        lam = (c + a * C0[0] + b * C0[1] - C0[2]) / (d[:, 2] - a * d[:, 0] - b * d[:, 1])
        depth, conf = _finish(lam, w, h, rng, holes)
        views.append({"K": K, "E": E, "depth": depth, "confidence": conf})
    dist = lambda P: (P[:, 2] - (a * P[:, 0] + b * P[:, 1] + c)) / np.sqrt(1 + a * a + b * b)
    return border, voxel, views, dist


BOXES = [(-4.0, -1.0, -3.0, 1.0, 3.0), (1.5, 5.0, 1.0, 4.5, 2.0)]   # x0, x1, y0, y1, height


def _box_hits(C0, d, x0, x1, y0, y1, z1):
    lo = np.array([x0, y0, 0.0])
    hi = np.array([x1, y1, z1])
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo - C0) / d
        t1 = (hi - C0) / d
    tn = np.nanmax(np.minimum(t0, t1), 1)
    tf = np.nanmin(np.maximum(t0, t1), 1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def boxes_scene(seed=1, w=64, h=48, holes=True):
    """Ground z = 0 with two boxes, a 16 x 12 m grid at 0.25 m whose size is not a multiple of 8 bricks' voxels in x and z."""
    rng = np.random.default_rng(seed)
    border, voxel = [-7.9, 7.1, -6.0, 6.0, -1.1, 4.3], 0.25
    views = []
    for k in range(8):
        C = (rng.uniform(-6, 6), rng.uniform(-5, 5), rng.uniform(11, 14))
        T = (rng.uniform(-3, 3), rng.uniform(-3, 3), 0.0)
        K = intrinsics(w, h, 0.7 * w)
        E = look_at(C, T)
        C0, d = rays(K, E, w, h)
        lam = np.where(d[:, 2] < 0, -C0[2] / d[:, 2], np.inf)
        for bx in BOXES:
            lam = np.minimum(lam, _box_hits(C0, d, *bx))
        depth, conf = _finish(lam, w, h, rng, holes)
        views.append({"K": K, "E": E, "depth": depth, "confidence": conf})

    def dist(P):
        best = np.abs(P[:, 2])
        for x0, x1, y0, y1, z1 in BOXES:
            q = np.stack([np.maximum(np.maximum(x0 - P[:, 0], P[:, 0] - x1), 0), np.maximum(np.maximum(y0 - P[:, 1], P[:, 1] - y1), 0),
                          np.maximum(np.maximum(0 - P[:, 2], P[:, 2] - z1), 0)], 1)
            inside = (P[:, 0] > x0) & (P[:, 0] < x1) & (P[:, 1] > y0) & (P[:, 1] < y1) & (P[:, 2] > 0) & (P[:, 2] < z1)
            dd = np.where(inside, np.minimum.reduce([P[:, 0] - x0, x1 - P[:, 0], P[:, 1] - y0, y1 - P[:, 1], P[:, 2], z1 - P[:, 2]]),
                          np.linalg.norm(q, axis=1))
            best = np.minimum(best, dd)
        return best

    return border, voxel, views, dist


SPHERE = (0.3, -0.2, 0.1, 2.0)


def sphere_scene(seed=2, w=56, h=56, holes=False, n=30):
    """A sphere of radius 2 m seen from n cameras on a sphere of radius 7 m around it; grid 6 x 6 x 6 m at 0.2 m."""
    rng = np.random.default_rng(seed)
    sx, sy, sz, r = SPHERE
    S = np.array([sx, sy, sz])
    border, voxel = [-2.9, 3.3, -3.2, 2.8, -3.0, 3.2], 0.2
    views = []
    gold = np.pi * (3 - np.sqrt(5))
    for k in range(n):
        zc = 1 - 2 * (k + 0.5) / n
        rc = np.sqrt(1 - zc * zc)
        C = S + 7.0 * np.array([rc * np.cos(gold * k), rc * np.sin(gold * k), zc])
        K = intrinsics(w, h, 0.9 * w)
        E = look_at(C, S + rng.uniform(-0.2, 0.2, 3))
        C0, d = rays(K, E, w, h)
        oc = C0 - S
        bq = (d @ oc)
        aq = (d * d).sum(1)
        disc = bq * bq - aq * (oc @ oc - r * r)
        lam = np.where(disc >= 0, (-bq - np.sqrt(np.maximum(disc, 0))) / aq, np.inf)
        depth, conf = _finish(lam, w, h, rng, holes)
        if not holes:
            conf = np.maximum(conf, 0.5).astype(np.float32)
        views.append({"K": K, "E": E, "depth": depth, "confidence": conf})
    return border, voxel, views, lambda P: np.linalg.norm(P - S, axis=1) - r


SCENES = {"plane": plane_scene, "boxes": boxes_scene, "sphere": sphere_scene}


def pipeline_settings(path, border, voxel, views_per_batch=None):
    return {"path": path, "border": border, "voxel": voxel, "trunc": None, "min_views": 2, "conf_threshold": 0.2,
            "views_per_batch": views_per_batch}


def main(out_dir, border, voxel):
    """One rank of a torch.distributed.run launch over pipeline_scene's block with the mesh stage on:
        python -m torch.distributed.run --nproc-per-node 2 tests/mesh_scene.py <out_dir> <Xmin,...,Zmax> <voxel>"""
    import os
    import sys

    import torch

    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import pipeline_scene as PS
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = PS.SceneViews()
    tm = {}
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              mesh=pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel, views_per_batch=3))
    print("rank %d/%d mesh %s" % (rank, world, "%.3f s" % tm["mesh_s"] if "mesh_s" in tm else "-"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    import sys

    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
