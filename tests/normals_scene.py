"""One rank of a torch.distributed.run launch for tests/test_normals_fusion_gpu.py: pipeline_scene's block, fused with normals
estimated from the gathered depth maps (pipeline.predict_and_fuse(estimate_normals=True)).

    python -m torch.distributed.run --nproc-per-node 2 tests/normals_scene.py <out_dir> <filter_sources 0|1> [views|scene_blocks]
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


def main(out_dir, filter_sources, fuse_partition="views"):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = PS.SceneViews()
    res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                                    fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=bool(filter_sources),
                                    fuse_partition=fuse_partition, estimate_normals=True,
                                    scene_blocks=PS.SCENE_BLOCKS if fuse_partition == "scene_blocks" else None)
    pipeline.save_fused(res, os.path.join(out_dir, "fused"))
    print("rank %d/%d fused %s with estimated normals" % (rank, world, [r["ref"] for r in res]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else "views")
