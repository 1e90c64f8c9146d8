"""cloud_scene's block with the merged cloud's outlier removal on, for tests/test_cloud_outliers_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/cloud_outliers_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <min_points>
        <radius> <k> <alpha | none> <min_neighbours>
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import cloud_scene as CS  # noqa: E402
import ortho_scene as OS  # noqa: E402
import pipeline_scene as PS  # noqa: E402


def run(out_dir, border, voxel, min_points, outliers, rank=0, world=1, timings=None):
    """cloud_scene.run with settings["outliers"] = outliers (None: the key is absent): this rank's results."""
    from deep3d_aerial_amd import pipeline

    scene = OS.ImageSceneViews()
    settings = CS.cloud_settings(os.path.join(out_dir, "cloud.ply"), border, voxel, min_points)
    if outliers is not None:
        settings["outliers"] = dict(outliers)
    return pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                                     fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=timings,
                                     cloud=settings)


def main(out_dir, border, voxel, min_points, outliers):
    from deep3d_aerial_amd import sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    tm = {}
    res = run(out_dir, border, voxel, min_points, outliers, rank, world, timings=tm)
    print("rank %d/%d fused %s, cloud %.3f s, outliers %s" % (rank, world, [r["ref"] for r in res], tm["cloud_s"], tm.get("cloud_outliers")))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), int(sys.argv[4]),
         {"radius": float(sys.argv[5]), "k": int(sys.argv[6]), "alpha": None if sys.argv[7] == "none" else float(sys.argv[7]),
          "min_neighbours": int(sys.argv[8])})
