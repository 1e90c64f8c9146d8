"""ortho_scene's block with the mesh and texture stages on, for tests/test_texture_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/texture_scene.py <out_dir> <Xmin,...,Zmax> <voxel>
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

import mesh_scene as MS  # noqa: E402
import ortho_scene as OS  # noqa: E402
import pipeline_scene as PS  # noqa: E402


def scene_border(scene, margin=1.0):
    """(border [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax], voxel) around the points the scene's depth maps see."""
    pts = []
    for v in scene.views:
        K, E = v["K"].astype(np.float64), v["E"].astype(np.float64)
        R, t = E[:3, :3], E[:3, 3]
        h, w = v["depth"].shape
        ys, xs = np.mgrid[0:h, 0:w]
        d = v["depth"].ravel().astype(np.float64)
        ok = np.isfinite(d) & (d > 0)
        rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        pts.append((R.T @ (rays[:, ok] * d[ok] - t[:, None])).T)
    P = np.concatenate(pts)
    lo, hi = np.floor(P.min(0)) - margin, np.ceil(P.max(0)) + margin
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2])], float((hi - lo).max()) / 96


def texture_settings(path, depth_tolerance=0.01, views_per_batch=None, page_size=256, pad=2):
    return {"path": path, "depth_tolerance": depth_tolerance, "views_per_batch": views_per_batch, "page_size": page_size, "pad": pad}


def main(out_dir, border, voxel):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = OS.ImageSceneViews()
    tm = {}
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              mesh=MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel),
                              texture=texture_settings(os.path.join(out_dir, "tex.ply"), views_per_batch=2))
    print("rank %d/%d texture %.3f s" % (rank, world, tm["texture_s"]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
