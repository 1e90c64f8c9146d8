"""Fusion with normals estimated from the depth maps (pipeline.predict_and_fuse(estimate_normals=True), predict --fuse_normals):
what the reference's fusion does when {view}_normal.pfm exists (fuse/fusion_3d_normal.py:437-443, 491-498) instead of the
default (0, 0, -1) camera-space normal."""
import os

import numpy as np
import pytest
import torch

import pipeline_scene as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(folder):
    out = {}
    for root, _, files in sorted(os.walk(folder)):
        for f in sorted(files):
            d = np.load(os.path.join(root, f))
            out[os.path.relpath(os.path.join(root, f[:-4]), folder)] = {k: d[k] for k in d.files}
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        for k in a[name]:
            assert np.array_equal(a[name][k], b[name][k]), (name, k)


def _vertex_normal_map(f, H, W):
    """fuse.extract_points' vertex normals put back on their pixels (skip_line = 1, no range clip: vertex k is the k-th
    confirmed pixel in row-major order)."""
    from deep3d_aerial_amd import fuse

    inf = [-np.inf, np.inf, -np.inf, np.inf]
    pts = fuse.extract_points(f["avg_xyz_world"], f["final_mask"], f["vis_infos"], None, f["normal_world"], inf, skip_line=1)
    fm = f["final_mask"].cpu().numpy()
    out = np.full((H, W, 3), np.nan, np.float32)
    out[fm] = pts["normal"].cpu().numpy()
    assert np.array_equal(out[fm], f["normal_world"].cpu().numpy()[fm])
    return out, fm


def test_vertex_normals_follow_the_surface():
    """A noise-free tilted plane: with estimated normals the vertex normals lie within 1 degree of the true world plane normal
    (vertices whose stencil touches a zero-depth hole excluded: points at the camera centre give the reference's meaningless
    normal there too); with the default normals the same vertices are the reference camera's viewing direction, ~4.9 degrees
    off, because the plane is tilted against it."""
    from deep3d_aerial_amd import fuse, pipeline, synthetic as S

    H, W = 96, 128
    ref, srcs = S.make_fusion_scene(H, W, 3, seed=7, noise=0.0)
    n_w = np.array([0.06, -0.04, -1.0])
    n_w /= np.linalg.norm(n_w)
    checker = fuse.ConsistencyChecker(1.0, 0.01, 10.0, 0.2)

    def views():
        v = {"ref": {"depth": _dev(ref["depth"]), "confidence": _dev(ref["confidence"]), "K": ref["K"], "E": ref["E"], "id": 1}}
        for i, s in enumerate(srcs):
            v["s%d" % i] = {"depth": _dev(s["depth"]), "K": s["K"], "E": s["E"], "id": i + 2}
        return v

    pairs = [{"ref": "ref", "src": ["s0", "s1", "s2"]}]
    est = pipeline.add_estimated_normals(views(), pairs, fusion_num=10, nei=1)
    assert all(v["normal"] is not None for v in est.values())
    f_est = fuse.fuse_block(est, pairs, checker, min_geo_consist_num=2, filter_sources=False)[0]
    f_def = fuse.fuse_block(views(), pairs, checker, min_geo_consist_num=2, filter_sources=False)[0]
    n_est, fm_est = _vertex_normal_map(f_est, H, W)
    n_def, fm_def = _vertex_normal_map(f_def, H, W)
    hole = ref["depth"] == 0
    near_hole = np.zeros_like(hole)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near_hole |= np.roll(np.roll(hole, dy, 0), dx, 1)
    near_hole[[0, -1], :] = True
    near_hole[:, [0, -1]] = True
    sel = fm_est & fm_def & ~near_hole
    assert sel.sum() > 2000, sel.sum()
    ang = lambda n: np.degrees(np.arccos(np.clip(n[sel].astype(np.float64) @ n_w / np.linalg.norm(n[sel], axis=-1), -1, 1)))
    a_est, a_def = ang(n_est), ang(n_def)
    print("estimated normals: max %.3f deg; default normals: min %.3f deg, over %d vertices" % (a_est.max(), a_def.min(), sel.sum()))
    assert a_est.max() < 1.0
    assert a_def.min() > 1.0


def _views_of(scene):
    recs = scene.view_records(PS.FUSION_NUM)
    return recs, {r["name"]: {"depth": _dev(v["depth"]), "confidence": _dev(v["confidence"]), "K": v["K"], "E": v["E"], "id": r["id"]}
                  for r, v in zip(recs, scene.views)}


def _run(tmp_path, tag, **kw):
    from deep3d_aerial_amd import pipeline

    scene = PS.SceneViews()
    return pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / tag), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                                     min_geo_consist_num=3, filter_sources=True, **kw)


def _assert_results_equal(a, b):
    assert [r["ref"] for r in a] == [r["ref"] for r in b]
    for x, y in zip(a, b):
        assert torch.equal(x["final_mask"], y["final_mask"]) and torch.equal(x["avg_xyz_world"], y["avg_xyz_world"]), x["ref"]
        for k in ("xyz", "normal", "views", "nviews"):
            assert torch.equal(x["points"][k], y["points"][k]), (x["ref"], k)


def test_predict_and_fuse_uses_the_kernel_normals_of_the_unfiltered_maps(tmp_path):
    """estimate_normals=True is fuse_block handed ops.normals_from_depth of every view's predicted (unfiltered) depth map as its
    "normal", bit for bit -- the source-filtering chain (filter on) does not reach the normals."""
    from deep3d_aerial_amd import fuse, ops

    got = _run(tmp_path, "est", estimate_normals=True)
    recs, views = _views_of(PS.SceneViews())
    for v in views.values():
        v["normal"] = ops.normals_from_depth(v["depth"], v["K"], nei=1)
    pairs = [{"ref": r["name"], "src": list(r["src"])[:PS.FUSION_NUM]} for r in recs]
    want = fuse.fuse_block(views, pairs, PS.checker(), fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True)
    inf = [-np.inf, np.inf, -np.inf, np.inf]
    assert [r["ref"] for r in got] == [f["ref"] for f in want]
    for r, f in zip(got, want):
        assert torch.equal(r["final_mask"], f["final_mask"]) and torch.equal(r["avg_xyz_world"], f["avg_xyz_world"])
        pts = fuse.extract_points(f["avg_xyz_world"], f["final_mask"], f["vis_infos"], None, f["normal_world"], inf, 2)
        for k in ("xyz", "normal", "views", "nviews"):
            assert torch.equal(r["points"][k], pts[k]), (r["ref"], k)
    # nei is honoured: another stencil, other normals
    got2 = _run(tmp_path, "est2", estimate_normals=True, normal_nei=2)
    assert any(not torch.equal(a["points"]["normal"], b["points"]["normal"]) for a, b in zip(got, got2))


def test_estimate_normals_off_changes_nothing(tmp_path):
    """estimate_normals=False is today's call, bit for bit (default normals), and estimated normals do change the vertices' normals."""
    from deep3d_aerial_amd import fuse

    today = _run(tmp_path, "today")
    off = _run(tmp_path, "off", estimate_normals=False)
    _assert_results_equal(today, off)
    recs, views = _views_of(PS.SceneViews())
    pairs = [{"ref": r["name"], "src": list(r["src"])[:PS.FUSION_NUM]} for r in recs]
    want = fuse.fuse_block(views, pairs, PS.checker(), fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=True)
    for r, f in zip(off, want):
        assert torch.equal(r["final_mask"], f["final_mask"]) and torch.equal(r["avg_xyz_world"], f["avg_xyz_world"])
    on = _run(tmp_path, "on", estimate_normals=True)
    assert sorted(os.listdir(tmp_path / "on")) == sorted(os.listdir(tmp_path / "today"))   # no new product without --save_normals
    default_dirs = [r["points"]["normal"] for r in today if len(r["points"]["normal"])]
    est_dirs = [r["points"]["normal"] for r in on if len(r["points"]["normal"])]
    assert default_dirs and est_dirs
    # the default normal of a view is one vector (its viewing direction); estimated ones vary with the noisy surface
    assert all(torch.equal(n, n[:1].expand_as(n)) for n in default_dirs)
    assert not all(torch.equal(n, n[:1].expand_as(n)) for n in est_dirs)


def _launch(n_ranks, out_dir, filter_sources, fuse_partition):
    import socket
    import subprocess
    import sys

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "normals_scene.py"), str(out_dir), str(int(filter_sources)), fuse_partition]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


@pytest.mark.parametrize("fuse_partition,filter_sources", [("views", False), ("scene_blocks", True)])
def test_two_ranks_fuse_what_one_rank_fuses_with_estimated_normals(tmp_path, fuse_partition, filter_sources):
    """Normals follow the view and the kernel is deterministic: two ranks on one GPU give the single-rank fused arrays byte for
    byte (the partitions under which that holds without normals: views with filtering off, scene blocks with it on)."""
    out1 = _launch(1, tmp_path / "one", filter_sources, fuse_partition)
    out2 = _launch(2, tmp_path / "two", filter_sources, fuse_partition)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    one, two = _load(tmp_path / "one" / "fused"), _load(tmp_path / "two" / "fused")
    assert len(one) >= PS.N_VIEWS
    _same(one, two)
    assert sum(len(v["xyz"]) for v in one.values()) > 2000
