"""One rank of a torch.distributed.run launch for tests/test_dsm_gpu.py: pipeline_scene's block, fused, and its DSM built on
rank 0 from every rank's points (pipeline.predict_and_fuse(dsm=...)).

    python -m torch.distributed.run --nproc-per-node 2 tests/dsm_scene.py <out_dir> <filter_sources 0|1> <views|scene_blocks> \
        <Xmin,Xmax,Ymin,Ymax> <unit>
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pipeline_scene as PS  # noqa: E402


def settings(path, border, unit):
    return {"path": path, "border": border, "unit": [unit, unit], "size": None, "select": "Robust_Max", "trim": 0.1,
            "min_points": 1, "interpolation": "MovingAverage", "radius": 2, "iterations": 1, "nodata": -9999.0}


def main(out_dir, filter_sources, fuse_partition, border, unit):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = PS.SceneViews()
    tm = {}
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=bool(filter_sources), timings=tm,
                                    fuse_partition=fuse_partition, dsm=settings(os.path.join(out_dir, "dsm.tif"), border, unit),
                                    scene_blocks=PS.SCENE_BLOCKS if fuse_partition == "scene_blocks" else None)
    pipeline.save_fused(res, os.path.join(out_dir, "fused"))
    print("rank %d/%d fused %s, dsm %.3f s" % (rank, world, [r["ref"] for r in res], tm["dsm_s"]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3], [float(v) for v in sys.argv[4].split(",")], float(sys.argv[5]))
