"""ortho_scene's block with the mesh and texture stages on, one view's image painted over and the outlier views rejected, for
tests/test_texture_outliers_gpu.py.

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/texture_outliers_scene.py <out_dir> <Xmin,...,Zmax> <voxel>
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

OUTLIERS = {"threshold": 0.06}
SMOOTH = {"weight": 0.1, "max_loss": 0.25, "rounds": 64}
PAINTED = 3   # the view whose image lies about the scene


def painted_scene(view=PAINTED):
    """ImageSceneViews with the central half of one view's image (255, 0, 255): what no other view shows there."""
    scene = OS.ImageSceneViews()
    img = scene.views[view]["image"]
    h, w = img.shape[:2]
    img[h // 4:h - h // 4, w // 4:w - w // 4] = (255, 0, 255)
    return scene


def main(out_dir, border, voxel):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = painted_scene()
    tm = {}
    settings = dict(TS.texture_settings(os.path.join(out_dir, "tex.ply"), views_per_batch=2), outliers=dict(OUTLIERS),
                    smooth_views=dict(SMOOTH))
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              mesh=MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel), texture=settings)
    print("rank %d/%d texture %.3f s" % (rank, world, tm["texture_s"]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
