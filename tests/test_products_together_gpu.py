"""Every product of pipeline.predict_and_fuse on at once writes what each product family writes alone: one joint run with the
cloud, the mesh (with the flip step), the DSM from the points, the orthophoto, the DTM with its nDSM, the objects with their table
and the texture with its orthophoto, against four runs with one family each.  It pins the order of the products and what one
hands to the next (the mesh to the texture, the DSM's raster to the orthophoto and the terrain step, the nDSM to the objects)."""
import os

import pytest
import torch

import dsm_scene
import mesh_scene as MS
import ortho_mesh_scene as OMS
import ortho_scene as OS
import pipeline_scene as PS
import texture_scene as TS

pytestmark = pytest.mark.gpu

FAMILIES = {"cloud": ("cloud",), "rasters": ("dsm", "ortho", "dtm", "objects"), "mesh": ("mesh",), "textured": ("mesh", "texture")}


def _settings(out, border, voxel):
    """Every product's settings with its files under `out`: the borders and units the product tests pass (scene_border's box and
    voxel, rasters of 0.5 m, the mesh orthophoto at 0.25 m), the terrain window and the object thresholds of test_objects_gpu (the
    scene is one tilted plane: its nDSM is 0 on the ground cells, so min_height 0 makes them the foreground)."""
    p = lambda name: os.path.join(out, name)
    return {"cloud": {"path": p("cloud.ply"), "border": list(border), "voxel": voxel, "min_points": 3},
            "mesh": dict(MS.pipeline_settings(p("mesh.ply"), border, voxel), flip={"max_angle": 30.0, "rounds": 2}),
            "dsm": dsm_scene.settings(p("dsm.tif"), border[:4], 0.5),
            "ortho": OS.ortho_settings(p("ortho.tif"), views_per_batch=2),
            "dtm": {"path": p("dtm.tif"), "ndsm": p("ndsm.tif"), "max_window": 8.5},
            "objects": {"path": p("objects.tif"), "table": p("objects.csv"), "min_height": 0.0, "min_area": 1.0, "connectivity": 8,
                        "open": 0.0},
            "texture": dict(TS.texture_settings(p("tex.ply"), views_per_batch=2), ortho=OMS.ortho_settings(p("tex_ortho.tif"), border, 0.25))}


def _listing(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(folder) for f in fs)


def test_all_products_together_write_what_each_family_writes_alone(tmp_path):
    from deep3d_aerial_amd import pipeline

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)

    def run(tag, keys):
        out = str(tmp_path / tag)
        s, tm = _settings(out, border, voxel), {}
        res = pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out, "MVS"), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                                        min_geo_consist_num=3, filter_sources=False, timings=tm, **{k: s[k] for k in keys})
        return res, tm

    joint, joint_tm = run("joint", sorted({k for keys in FAMILIES.values() for k in keys}))
    files = _listing(tmp_path / "joint")
    assert len(joint) > 0 and sum(int(r["points"]["xyz"].shape[0]) for r in joint) > 1000
    table = (tmp_path / "joint" / "objects.csv").read_text().splitlines()
    assert len(table) >= 2, table                                   # a header and at least one object: the files compared are not empty
    seen, keys = set(), set()
    for tag, family in FAMILIES.items():
        res, tm = run(tag, family)
        alone = _listing(tmp_path / tag)
        assert set(alone) <= set(files) and len(alone) > len([f for f in alone if f.startswith("MVS")]), (tag, alone)
        for name in alone:
            assert (tmp_path / tag / name).read_bytes() == (tmp_path / "joint" / name).read_bytes(), (tag, name)
        assert [r["ref"] for r in res] == [r["ref"] for r in joint]
        for a, b in zip(res, joint):
            assert torch.equal(a["final_mask"], b["final_mask"]), (tag, a["ref"])
            for k in ("xyz", "normal"):
                assert torch.equal(a["points"][k], b["points"][k]), (tag, a["ref"], k)
        seen |= set(alone)
        keys |= set(tm)
    assert seen == set(files)                                        # no file of the joint run is left uncompared
    for name in ("cloud.ply", "mesh.ply", "dsm.tif", "dsm.tfw", "ortho.tif", "dtm.tif", "ndsm.tif", "objects.tif", "objects.csv", "tex.ply",
                 "tex_ortho.tif"):
        assert name in files, name
    assert set(joint_tm) == keys
    assert {"cloud_s", "mesh_s", "mesh_flip_s", "dsm_s", "ortho_s", "dtm_s", "objects_s", "texture_s", "texture_ortho_s"} <= keys
