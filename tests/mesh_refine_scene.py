"""pipeline_scene's block with sharp images and a mesh to refine, for tests/test_mesh_refine.py and tests/test_mesh_refine_gpu.py.

The views are pipeline_scene's (7 views of 96 x 128 over one tilted plane).  Every image is the world texture `texture` at the
point where the pixel's ray meets the TRUE plane, so the images are photo-consistent across views exactly on that plane; the world
texture has periods of a few pixels, and a disc of it is painted uniform.  The mesh is a grid triangulation of the plane, 37 x 29
vertices (not a multiple of the 16 vertices a workgroup of the match holds), whose active vertices are pushed off the plane along
their normals by a seeded amount within 0.75 * reach * step; plus a vertex that only a degenerate face uses and a vertex no face
uses.  The grid reaches past the images on one side, so some vertices are seen by fewer than two views and some patches leave an
image.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/mesh_refine_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <step>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pipeline_scene as PS  # noqa: E402

# the plane of synthetic.make_fusion_scene: n_w . X = n_w . (0, 0, 600)
PLANE_N = np.array([0.06, -0.04, -1.0]) / np.linalg.norm([0.06, -0.04, -1.0])
PLANE_C = float(PLANE_N @ np.array([0.0, 0.0, 600.0]))
NX, NY = 37, 29
X_RANGE, Y_RANGE = (-260.0, 150.0), (-110.0, 110.0)
UNIFORM = (60.0, 20.0, 22.0)   # centre x, y and radius of the disc painted one colour
# the scene's settings: a pixel is about 3.35 world units on the plane
STEP, SPACING, REACH = 5.0, 4.0, 4
SETTINGS = {"step": STEP, "spacing": SPACING}
SEED = 23


def texture(x, y):
    """The world texture: three channels of a few pixels' period, uniform inside the disc."""
    t = np.stack([128 + 90 * np.sin(x / 2.3) * np.cos(y / 3.1), 128 + 90 * np.cos(x / 3.7 + y / 2.9), 128 + 90 * np.sin((x - y) / 2.6)], -1)
    inside = (x - UNIFORM[0]) ** 2 + (y - UNIFORM[1]) ** 2 <= UNIFORM[2] ** 2
    t[inside] = (120.0, 130.0, 110.0)
    return t


def plane_z(x, y):
    return (PLANE_N[0] * x + PLANE_N[1] * y - PLANE_C) / -PLANE_N[2]


class RefineSceneViews(PS.SceneViews):
    """pipeline_scene's views with images rendered on the true plane (the depth maps keep their noise and holes)."""

    def __init__(self, *args, **kwargs):
        super(RefineSceneViews, self).__init__(*args, **kwargs)
        for v in self.views:
            K, E = v["K"].astype(np.float64), v["E"].astype(np.float64)
            R, t = E[:3, :3], E[:3, 3]
            C = -R.T @ t
            ys, xs = np.mgrid[0:self.h, 0:self.w]
            rays = R.T @ (np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(self.h * self.w)]))
            lam = (PLANE_C - PLANE_N @ C) / (PLANE_N @ rays)
            P = (C[:, None] + rays * lam).T
            v["image"] = np.clip(np.floor(texture(P[:, 0], P[:, 1]) + 0.5), 0, 255).astype(np.uint8).reshape(self.h, self.w, 3)

    def __getitem__(self, idx):
        item = super(RefineSceneViews, self).__getitem__(idx)
        item["outimage"] = self.views[idx]["image"]
        return item


def numpy_views(scene=None):
    """The views as the numpy restatements take them: dicts with id, K, E, depth, image."""
    scene = scene or RefineSceneViews()
    return [dict(v, id=i) for i, v in enumerate(scene.views)]


def grid_mesh():
    """(V [n, 3] fp64 on the plane, F [m, 3] int32, grid [NY, NX] of vertex indices, extra: the indices of the vertex with only a
    degenerate face and of the unreferenced vertex).  The normals look at the cameras (-Z)."""
    xs, ys = np.linspace(X_RANGE[0], X_RANGE[1], NX), np.linspace(Y_RANGE[0], Y_RANGE[1], NY)
    gx, gy = np.meshgrid(xs, ys)
    V = np.stack([gx.ravel(), gy.ravel(), plane_z(gx.ravel(), gy.ravel())], 1)
    idx = np.arange(NX * NY).reshape(NY, NX)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    F = np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, d], 1)]).astype(np.int32)
    n = NX * NY
    lone = np.array([[X_RANGE[1] + 10.0, 0.0, plane_z(X_RANGE[1] + 10.0, 0.0)], [X_RANGE[1] + 20.0, 0.0, plane_z(X_RANGE[1] + 20.0, 0.0)]])
    V = np.concatenate([V, lone])
    F = np.concatenate([F, np.array([[n, n, idx[NY // 2, NX - 1]]], np.int32)])   # a face with a repeated index, hung on the border
    return V, F, idx, (n, n + 1)


def displaced_mesh(amplitude=0.75 * REACH * STEP, seed=SEED):
    """(V0 [n, 3] fp32: the grid pushed off the plane, F, true [n, 3] fp64, interior [n] bool: the grid's vertices off its border).
    Every interior vertex moves along the plane's normal by a seeded amount in -amplitude .. amplitude."""
    V, F, idx, _ = grid_mesh()
    interior = np.zeros(len(V), bool)
    interior[idx[1:-1, 1:-1].ravel()] = True
    rng = np.random.default_rng(seed)
    off = rng.uniform(-amplitude, amplitude, len(V)) * interior
    return (V + off[:, None] * PLANE_N[None, :]).astype(np.float32), F, V, interior


def plane_distance(V):
    """|n_w . X - c| per vertex, fp64."""
    return np.abs(np.asarray(V, np.float64) @ PLANE_N - PLANE_C)


def mesh_border(scene):
    """(border, voxel) of the mesh stage over the block, as texture_scene.scene_border gives them."""
    import texture_scene as TS

    return TS.scene_border(scene)


def main(out_dir, border, voxel, step):
    import mesh_scene as MS
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = RefineSceneViews()
    tm = {}
    mesh = dict(MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel), refine={"step": step, "views_per_batch": 2})
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm, mesh=mesh)
    if rank == 0:
        print("rank %d/%d mesh_refine %.3f s" % (rank, world, tm["mesh_refine_s"]))
    else:
        print("rank %d/%d" % (rank, world))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), float(sys.argv[4]))
