"""ortho_scene's block with the mesh and texture stages and the orthophoto of the textured mesh on, for
tests/test_ortho_mesh_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/ortho_mesh_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <unit>
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


def ortho_settings(path, border, unit):
    """The scene's cameras look along +Z: they are on the low-Z side, so the lowest surface is the one they see."""
    return {"path": path, "border": list(border[:4]), "unit": [unit, unit], "size": None, "z_down": True}


def main(out_dir, border, voxel, unit):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = OS.ImageSceneViews()
    tm = {}
    tex = dict(TS.texture_settings(os.path.join(out_dir, "tex.ply"), views_per_batch=2),
               ortho=ortho_settings(os.path.join(out_dir, "ortho.tif"), border, unit))
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              mesh=MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel), texture=tex)
    print("rank %d/%d texture %.3f s, ortho %s" % (rank, world, tm["texture_s"],
                                                   "%.3f s" % tm["texture_ortho_s"] if "texture_ortho_s" in tm else "-"))
    if rank == 0:
        assert 0 < tm["texture_ortho_s"] <= tm["texture_s"]
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), float(sys.argv[4]))
