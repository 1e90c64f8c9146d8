"""ortho_scene's block (pipeline_scene's views with rendered images) with the merged point cloud on, for
tests/test_cloud_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/cloud_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <min_points>
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ortho_scene as OS  # noqa: E402
import pipeline_scene as PS  # noqa: E402


def cloud_settings(path, border, voxel, min_points=1):
    return {"path": path, "border": list(border), "voxel": voxel, "min_points": int(min_points)}


def run(out_dir, border, voxel, min_points, rank=0, world=1, cloud=True, timings=None):
    """predict_and_fuse on the scene with filter_sources off (the fused points then do not depend on the number of ranks):
    this rank's results."""
    from deep3d_aerial_amd import pipeline

    scene = OS.ImageSceneViews()
    settings = cloud_settings(os.path.join(out_dir, "cloud.ply"), border, voxel, min_points) if cloud else None
    return pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                                     fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=timings,
                                     cloud=settings)


def main(out_dir, border, voxel, min_points):
    from deep3d_aerial_amd import sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    tm = {}
    res = run(out_dir, border, voxel, min_points, rank, world, timings=tm)
    print("rank %d/%d fused %s, cloud %.3f s" % (rank, world, [r["ref"] for r in res], tm["cloud_s"]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), int(sys.argv[4]))
