"""ortho_scene's block with the mesh stage (one smoothing iteration, then decimation) and the texture stage on, for
tests/test_mesh_decimate_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/mesh_decimate_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <ratio>
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_scene as MS  # noqa: E402
import ortho_scene as OS  # noqa: E402
import pipeline_scene as PS  # noqa: E402
import texture_scene as TS  # noqa: E402


def mesh_settings(path, border, voxel, ratio):
    s = MS.pipeline_settings(path, border, voxel)
    s.update(smooth=1, decimate=ratio)
    return s


def run(out_dir, border, voxel, ratio, rank=0, world=1):
    from deep3d_aerial_amd import pipeline

    scene = OS.ImageSceneViews()
    tm = {}
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              mesh=mesh_settings(os.path.join(out_dir, "mesh.ply"), border, voxel, ratio),
                              texture=TS.texture_settings(os.path.join(out_dir, "tex.ply"), views_per_batch=2))
    return tm


def main(out_dir, border, voxel, ratio):
    from deep3d_aerial_amd import sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    tm = run(out_dir, border, voxel, ratio, rank, world)
    print("rank %d/%d mesh %s" % (rank, world, "%.3f s" % tm["mesh_s"] if "mesh_s" in tm else "-"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), float(sys.argv[4]))
