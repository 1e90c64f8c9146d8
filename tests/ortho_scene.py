"""pipeline_scene's block with rendered images, for the orthophoto stage (tests/test_ortho_gpu.py): every view's reference image
is the texture of the world point its depth map sees, in the reference's item layout ("outimage").

Run as a script it is one rank of a torch.distributed.run launch:
    python -m torch.distributed.run --nproc-per-node 2 tests/ortho_scene.py <out_dir> <Xmin,Xmax,Ymin,Ymax> <unit>
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

import dsm_scene  # noqa: E402
import pipeline_scene as PS  # noqa: E402


def texture(x, y):
    return np.stack([128 + 100 * np.sin(x / 3.0), 128 + 100 * np.cos(y / 4.0), 128 + 60 * np.sin((x - y) / 5.0)], -1)


class ImageSceneViews(PS.SceneViews):
    def __init__(self, *args, **kwargs):
        super(ImageSceneViews, self).__init__(*args, **kwargs)
        for v in self.views:
            K, E = v["K"].astype(np.float64), v["E"].astype(np.float64)
            R, t = E[:3, :3], E[:3, 3]
            ys, xs = np.mgrid[0:self.h, 0:self.w]
            rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(self.h * self.w)])
            P = (R.T @ (rays * v["depth"].ravel().astype(np.float64) - t[:, None])).T
            v["image"] = np.clip(np.floor(texture(P[:, 0], P[:, 1]) + 0.5), 0, 255).astype(np.uint8).reshape(self.h, self.w, 3)

    def __getitem__(self, idx):
        item = super(ImageSceneViews, self).__getitem__(idx)
        item["outimage"] = self.views[idx]["image"]
        return item


def ortho_settings(path, depth_tolerance=0.01, views_per_batch=None):
    return {"path": path, "depth_tolerance": depth_tolerance, "views_per_batch": views_per_batch}


def main(out_dir, border, unit):
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = ImageSceneViews()
    tm = {}
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm,
                              dsm=dsm_scene.settings(os.path.join(out_dir, "dsm.tif"), border, unit),
                              ortho=ortho_settings(os.path.join(out_dir, "ortho.tif"), views_per_batch=2))
    print("rank %d/%d ortho %.3f s" % (rank, world, tm["ortho_s"]))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
