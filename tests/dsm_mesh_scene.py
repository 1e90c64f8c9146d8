"""One rank of a torch.distributed.run launch for tests/test_dsm_mesh_gpu.py: ortho_scene's textured block, its mesh built on rank 0
and the DSM rasterised from that mesh there (pipeline.predict_and_fuse(mesh=..., dsm={"source": "mesh", ...})), with the
orthophoto draped on it.

    python -m torch.distributed.run --nproc-per-node 2 tests/dsm_mesh_scene.py <out_dir> <Xmin,Xmax,Ymin,Ymax,Zmin,Zmax> <voxel>
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


def settings(path, border, unit, interpolation=None):
    """DSM settings of the mesh source on the XY part of the mesh border."""
    return {"path": path, "border": list(border[:4]), "unit": [unit, unit], "size": None, "select": "Max", "trim": 0.1,
            "min_points": 1, "interpolation": interpolation, "radius": 2, "iterations": 1, "nodata": -9999.0, "source": "mesh"}


def run(out_dir, border, voxel, rank=0, world=1, timings=None):
    from deep3d_aerial_amd import pipeline

    scene = OS.ImageSceneViews()
    return pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                                     fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=timings,
                                     mesh=MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel),
                                     dsm=settings(os.path.join(out_dir, "dsm.tif"), border, voxel),
                                     ortho=OS.ortho_settings(os.path.join(out_dir, "ortho.tif")))


def main(out_dir, border, voxel):
    from deep3d_aerial_amd import sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    tm = {}
    run(out_dir, border, voxel, rank, world, tm)
    print("rank %d/%d dsm %s" % (rank, world, "%.3f s" % tm["dsm_s"] if "dsm_s" in tm else "-"))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
