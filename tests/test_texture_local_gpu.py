"""The local seam levelling kernels (csrc/texture_local.hip) on the GPU: seam edges, sorted records, D, the distances, the
corrections after 1, 4 and 512 sweeps and the levelled pages bit-equal to the numpy restatement of tests/test_texture_local.py;
both solve paths (the chart in LDS, global sweeps) give the same bits; independence of runs, view order and batching; the gain
and offset scene alone and after the global levelling; and the option through the pipeline on one and two ranks, predict and the
standalone command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import pipeline_scene as PS
import test_texture_gpu as G
import test_texture_level as L
import test_texture_level_gpu as LG
import test_texture_local as LC
import texture_scene as TS

ROOT = G.ROOT
pytestmark = pytest.mark.gpu
SCENES = [(0, 16, 3), (1, 24, 4), (3, 24, 2)]   # the sizes the global levelling's tests use, page size 256


@functools.lru_cache(maxsize=None)
def _reference(seed, n, n_views):
    """The scene, its layout, pages and coverage by the restatement (test_texture_level_gpu's, shared) and the local levelling of
    those pages by the restatement, with c after 1 and 4 sweeps; shared and never changed."""
    V, F, vs, key, want = LG._reference(seed, n, n_views)
    return V, F, vs, key, want, LC.local_numpy(V, F, want, vs, want["atlas"], snapshots=(1, 4))


def _fields(state):
    from deep3d_aerial_amd import texture

    c, dist, domain, seam = texture.local_fields(state)
    return c.cpu().numpy().astype(np.int64), dist.cpu().numpy(), domain.cpu().numpy(), seam.cpu().numpy()


def _gpu_state(seed, n, n_views):
    """The GPU's layout and filled atlas of a scene, and the state after the fold."""
    from deep3d_aerial_amd import texture

    V, F, vs, key, want, loc = _reference(seed, n, n_views)
    v, f, ov, gkey, chart, packing, table, atlas = LG._gpu_layout(V, F, vs)
    seams = texture.local_seams(f, chart, len(V))
    texel, rec = texture.local_samples(v, seams, table, packing, ov, atlas)
    cover = texture.level_coverage(v, f, chart, table, packing, ov)
    return v, f, ov, gkey, chart, packing, table, atlas, seams, texel, rec, cover, texture.local_fold(texel, rec, cover, packing)


@pytest.mark.parametrize("seed,n,n_views", SCENES)
def test_seams_records_fold_and_band_are_bit_equal_to_numpy(seed, n, n_views):
    from deep3d_aerial_amd import texture

    V, F, vs, key, want, loc = _reference(seed, n, n_views)
    # what the scene must hold for the test to mean something
    gw, P = want["graph"], want["packing"].page_size
    wh = np.array([(b[2], b[3]) for b in loc["boxes"]])
    assert len(loc["seams"]) >= 1 and (np.bincount(gw["nodes"] % gw["n"]) >= 3).any()
    assert ((wh[:, 0] > 64) | (wh[:, 1] > 8)).any() and any(b[0] == 0 or b[0] + b[2] == P for b in loc["boxes"])
    assert len(np.unique(loc["samples"]["texel"])) < len(loc["samples"]["texel"])   # texels with more than one record
    v, f, ov, gkey, chart, packing, table, atlas, seams, texel, rec, cover, state = _gpu_state(seed, n, n_views)
    covered = want["cover"] != L.EMPTY
    assert np.array_equal(chart.cpu().numpy(), want["chart"]) and np.array_equal(LG._rgb(atlas)[covered], want["atlas"][covered])
    assert np.array_equal(seams.cpu().numpy(), loc["seams"])
    assert np.array_equal(texel.cpu().numpy(), loc["samples"]["texel"]) and np.array_equal(rec.cpu().numpy(), loc["samples"]["rec"])
    c, dist, domain, seam = _fields(state)
    assert np.array_equal(domain, want["cover"] != L.EMPTY) and np.array_equal(seam, loc["state"]["seam"])
    assert np.array_equal(c, loc["D"]) and np.array_equal(dist, np.where(seam, 0, LC.FAR))
    for lds_texels in (None, 0):
        banded = texture.local_band(state.clone(), table, packing, 16, lds_texels=lds_texels)
        c2, dist, domain2, seam2 = _fields(banded)
        assert np.array_equal(dist, loc["state"]["dist"]) and np.array_equal(c2, loc["D"])
        assert np.array_equal(domain2, domain) and np.array_equal(seam2, seam)
    assert ((dist >= 1) & (dist <= 16)).sum() > 500 and (domain & (dist == LC.FAR)).any()
    # the seam edges reuse the (edge, face) pairs of the global levelling's graph: the same arrays either way
    pairs = texture.level_edge_pairs(f, chart, len(V))
    assert torch.equal(texture.local_seams(f, chart, len(V), pairs), seams)
    LG._check_graph(texture.level_graph(f, chart, len(V), pairs=pairs), gw)


@pytest.mark.parametrize("seed,n,n_views", SCENES)
def test_both_solve_paths_are_bit_equal_to_numpy_after_1_4_and_512_sweeps(seed, n, n_views):
    from deep3d_aerial_amd import texture

    V, F, vs, key, want, loc = _reference(seed, n, n_views)
    v, f, ov, gkey, chart, packing, table, atlas, seams, texel, rec, cover, state = _gpu_state(seed, n, n_views)
    sizes = (table[:, 2].astype(np.int64) * table[:, 3]).tolist()
    median = int(np.median(sizes))
    n_charts = len(sizes)
    assert 16 < loc["sweeps"] < 512   # the global path reads its counts more than once, and the fixed point ends the solve
    for iterations, want_c in ((1, loc["snaps"][1]), (4, loc["snaps"][4]), (512, loc["state"]["c"])):
        for lds_texels, split in ((None, (n_charts, 0)), (0, (0, n_charts)), (median, None)):
            solved, info = texture.local_solve(state.clone(), table, packing, 16, iterations, lds_texels=lds_texels)
            c, dist, domain, seam = _fields(solved)
            assert np.array_equal(c, want_c), (iterations, lds_texels)
            assert np.array_equal(dist, loc["state"]["dist"])
            if split is None:
                assert info["charts_lds"] > 0 and info["charts_global"] > 0 and info["charts_lds"] + info["charts_global"] == n_charts
            else:
                assert (info["charts_lds"], info["charts_global"]) == split
            assert info["sweeps"] == min(iterations, loc["sweeps"]) and info["converged"] == (iterations > loc["sweeps"])
    assert (loc["state"]["c"] != loc["snaps"][4]).any() and (loc["snaps"][4] != loc["snaps"][1]).any()
    assert not loc["state"]["c"][loc["state"]["dist"] == LC.FAR].any()


@pytest.mark.parametrize("seed,n,n_views", SCENES)
def test_the_levelled_pages_are_bit_equal_to_numpy(seed, n, n_views):
    from deep3d_aerial_amd import texture

    V, F, vs, key, want, loc = _reference(seed, n, n_views)
    v, f, ov, gkey, chart, packing, table, atlas = LG._gpu_layout(V, F, vs)
    alpha = atlas.clone() & -16777216   # 0xff000000 as int32
    info = texture.local_pages(v, f, gkey, chart, table, packing, ov, atlas, 16, 512)
    st = loc["state"]
    assert info == {"seam_edges": len(loc["seams"]), "seam_texels": int(st["seam"].sum()),
                    "active": int((st["domain"] & (st["dist"] >= 1) & (st["dist"] <= 16)).sum()), "sweeps": loc["sweeps"], "converged": True}
    assert torch.equal(atlas & -16777216, alpha)
    got = LG._rgb(texture.finish_pages(atlas))
    assert np.array_equal(got, loc["levelled"]) and (got != want["atlas"]).any()
    # through texture_mesh, with the global step's coverage reused when both run
    res = texture.texture_mesh(v, f, ov, page_size=256, local={})
    assert np.array_equal(L.stack_pages(res["pages"]), loc["levelled"]) and res["local"] == info and "level" not in res
    both = texture.texture_mesh(v, f, ov, page_size=256, level={}, local={"radius": 16, "iterations": 512})
    glob = texture.texture_mesh(v, f, ov, page_size=256, level={})
    again = LC.local_numpy(V, F, want, vs, L.stack_pages(glob["pages"]))
    assert np.array_equal(L.stack_pages(both["pages"]), again["levelled"]) and both["level"] == glob["level"]
    assert torch.equal(both["texcoord"], glob["texcoord"]) and torch.equal(both["texnumber"], glob["texnumber"])


# ----------------------------------------------------------------------------------------
# the scene whose views differ in gain and offset
# ----------------------------------------------------------------------------------------
def _step(V, vs, want, seams, pages):
    """The mean absolute colour step over the seam samples, with the restatement's taps on `pages`."""
    return LC.seam_step(LC.samples_numpy(V, seams, want["rects"], want["packing"], want["ids"], vs, L.stack_pages(pages))["diff"])


def test_local_levelling_clears_the_seams_of_the_gain_scene_alone_and_after_the_global_step():
    """The mean absolute step over all seam samples, taken with the same taps on the pages: 40.89 levels before; the restatement
    gives 3.77 after the local step alone (the condition: at most half), 11.78 after the global step alone and 3.40 after both
    (the condition: no larger than after the global step alone)."""
    from deep3d_aerial_amd import texture

    V, F, vs = LG._gain_scene()
    key, want, _ = LG._gain_reference()
    seams = LC.seams_numpy(F, want["chart"])
    v, f = G._mesh(V, F)
    plain = texture.texture_mesh(v, f, G._views(vs), page_size=256)
    local = texture.texture_mesh(v, f, G._views(vs), page_size=256, local={})
    glob = texture.texture_mesh(v, f, G._views(vs), page_size=256, level={})
    both = texture.texture_mesh(v, f, G._views(vs), page_size=256, level={}, local={})
    assert np.array_equal(plain["key"].cpu().numpy(), key) and local["local"]["seam_edges"] == len(seams) > 10
    assert local["local"]["converged"] and both["local"]["converged"] and "level" not in local and "local" not in glob
    before, after_local, after_global, after_both = (_step(V, vs, want, seams, r["pages"]) for r in (plain, local, glob, both))
    print("seam step over %d edges: %.2f before, %.2f local alone (%d sweeps), %.2f global alone, %.2f global then local (%d sweeps)" %
          (len(seams), before, after_local, local["local"]["sweeps"], after_global, after_both, both["local"]["sweeps"]))
    assert after_local <= 0.5 * before
    assert after_both <= after_global
    # the local step alone is the restatement's, bit for bit
    assert np.array_equal(L.stack_pages(local["pages"]), LC.local_numpy(V, F, want, vs, want["atlas"])["levelled"])
    for r in (local, glob, both):
        assert torch.equal(r["texcoord"], plain["texcoord"]) and torch.equal(r["texnumber"], plain["texnumber"])


def test_two_runs_view_order_and_batching_give_the_same_pages_and_off_changes_nothing():
    from deep3d_aerial_amd import texture

    V, F, vs = LG._gain_scene()
    v, f = G._mesh(V, F)
    first = None
    for vpb, order in ((None, vs), (None, vs), (1, vs[::-1]), (3, [vs[i] for i in (3, 0, 6, 1, 2, 5, 4)])):
        res = texture.texture_mesh(v, f, G._views(order), views_per_batch=vpb, page_size=256, local={"radius": 12})
        pages = L.stack_pages(res["pages"])
        first = pages if first is None else first
        assert np.array_equal(pages, first)
    # local=None is today's call, and one chart only has no seam: the pages stay byte for byte
    a = texture.texture_mesh(v, f, G._views(vs), 0.01, None, 256, 2, texture.EMPTY_COLOR, level={})
    b = texture.texture_mesh(v, f, G._views(vs), 0.01, None, 256, 2, texture.EMPTY_COLOR, level={}, local=None)
    assert "local" not in b and set(a) == set(b) and all(np.array_equal(x, y) for x, y in zip(a["pages"], b["pages"]))
    assert (L.stack_pages(a["pages"]) != first).any()
    one = texture.texture_mesh(v, f, G._views(vs[:1]), page_size=256)
    lev = texture.texture_mesh(v, f, G._views(vs[:1]), page_size=256, local={})
    assert lev["local"] == {"seam_edges": 0, "seam_texels": 0, "active": 0, "sweeps": 0, "converged": True}
    assert all(np.array_equal(x, y) for x, y in zip(one["pages"], lev["pages"]))


def test_local_inputs_are_checked():
    from deep3d_aerial_amd import texture

    V, F, vs, key, want, loc = _reference(0, 16, 3)
    v, f, ov, gkey, chart, packing, table, atlas = LG._gpu_layout(V, F, vs)
    args = lambda a: (v, f, gkey, chart, table, packing, ov, a)
    with pytest.raises(ValueError):
        texture.local_pages(*args(atlas[:-1]))
    with pytest.raises(RuntimeError):
        texture.local_pages(*args(atlas.cpu()))
    with pytest.raises(RuntimeError):
        texture.local_seams(f.cpu(), chart.cpu(), len(V))
    for bad in ({"radius": 0}, {"radius": 255}, {"iterations": 0}, {"iterations": 65536}):
        with pytest.raises(ValueError):
            texture.local_pages(*args(atlas), **bad)
        with pytest.raises(ValueError):
            texture.texture_mesh(v, f, ov, page_size=256, local=bad)
    state = torch.zeros_like(atlas, dtype=torch.int64)
    with pytest.raises(ValueError):
        texture.local_solve(state[:-1], table, packing)
    with pytest.raises(ValueError):
        texture.local_solve(state, table, packing, lds_texels=-1)
    with pytest.raises(RuntimeError):
        texture.local_solve(state.cpu(), table, packing)


# ----------------------------------------------------------------------------------------
# the pipeline stage and the command lines
# ----------------------------------------------------------------------------------------
LOCAL_SCENE = LG.LEVEL_SCENE.replace('level = {} if sys.argv[4] == "1" else None',
                                     'level = {} if sys.argv[4] == "1" else None\nlocal = {"radius": 12}').replace(
    "level=level)", "level=level, local=local)")


def test_two_ranks_write_the_locally_levelled_mesh_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import texture

    assert "local=local" in LOCAL_SCENE and 'local = {"radius": 12}' in LOCAL_SCENE
    script = tmp_path / "local_scene.py"
    script.write_text(LOCAL_SCENE % (ROOT, os.path.join(ROOT, "tests")))
    border, voxel = TS.scene_border(OS.ImageSceneViews())
    LG._launch(1, tmp_path / "one", border, voxel, script, True)
    LG._launch(2, tmp_path / "two", border, voxel, script, True)
    _, _, _, _, files = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    for name in ["tex.ply", "mesh.ply"] + files:
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    # texture_mesh on the mesh and MVS folder the stage wrote, the images as files: the stage's pages with both steps, other
    # pages with the global step alone (this fails when the stage drops the local step)
    from PIL import Image
    from deep3d_aerial_amd import mesh, ortho

    (tmp_path / "images").mkdir()
    for i, v in enumerate(LG._gain_scene()[2]):
        Image.fromarray(v["image"]).save(str(tmp_path / "images" / ("scene_%02d.png" % i)))
    mv, mf = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    views = ortho.load_mvs_views(str(tmp_path / "one" / "MVS"), str(tmp_path / "images"))
    v, f = torch.from_numpy(mv).cuda(), torch.from_numpy(mf).cuda()
    both = texture.texture_mesh(v, f, views, page_size=256, level={}, local={"radius": 12})
    glob = texture.texture_mesh(v, f, views, page_size=256, level={})
    assert both["local"]["seam_edges"] > 0 and len(files) == len(both["pages"])
    for name, page in zip(files, both["pages"]):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "one" / name)).convert("RGB")), page), name
    assert any((a != b).any() for a, b in zip(both["pages"], glob["pages"]))


def test_predict_main_texture_level_local_and_the_standalone_level_local_flag(tmp_path, monkeypatch):
    """predict.main --fuse --mesh --texture --texture_level_local on the gain and offset scene (entering predict.main as in
    test_texture_level_gpu), python -m deep3d_aerial_amd.texture --level_local on the mesh and MVS folder it wrote, and
    texture_mesh(local={...}) on the same mesh and views: the same pages from all three, other pages without the flag."""
    from PIL import Image
    from deep3d_aerial_amd import mesh, ortho, predict as P, texture

    scene = OS.ImageSceneViews()
    for v, (gain, offset) in zip(scene.views, LG.GAINS):
        v["image"] = np.clip(np.rint(v["image"].astype(np.float64) * gain + offset), 0, 255).astype(np.uint8)
    monkeypatch.setattr(P, "SyntheticBlock", lambda *a, **k: scene)
    monkeypatch.setattr(P, "build_model", lambda *a, **k: PS.SceneModel(scene))
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    border, voxel = TS.scene_border(scene)
    tflags = ["--depth_tolerance=0.01", "--page_size=256", "--views_per_batch=2"]
    lflags = ["--level_local", "--level_local_radius=10", "--level_local_iterations=300"]

    def run(out, extra):
        P.main(["--synthetic_items", str(len(scene)), "--output_folder", str(out / "MVS"), "--display", "False", "--fuse",
                "--fuse_filter_sources=0", "--fusion_num", str(PS.FUSION_NUM), "--geo_consist_num=3", "--position_threshold=1.0",
                "--depth_threshold=0.01", "--normal_threshold=10.0", "--photometric_threshold=0.2", "--mesh", str(out / "mesh.ply"),
                "--mesh_border=" + ",".join(repr(b) for b in border), "--mesh_voxel=" + repr(voxel), "--mesh_min_views=2",
                "--mesh_conf_threshold=0.2", "--texture", str(out / "tex.ply")] + ["--texture_" + f[2:] for f in tflags + extra])
        return texture.read_textured_ply(str(out / "tex.ply"))

    _, F, _, _, files = run(tmp_path / "local", lflags)
    _, _, _, _, files_plain = run(tmp_path / "plain", [])
    assert len(F) > 100 and files and files == files_plain
    assert (tmp_path / "plain" / "tex.ply").read_bytes() == (tmp_path / "local" / "tex.ply").read_bytes()   # no texcoord moves
    assert [name for name in files if (tmp_path / "plain" / name).read_bytes() != (tmp_path / "local" / name).read_bytes()]
    (tmp_path / "images").mkdir()
    for i, v in enumerate(scene.views):
        Image.fromarray(v["image"]).save(str(tmp_path / "images" / ("scene_%02d.png" % i)))
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.texture", "--mesh", str(tmp_path / "local" / "mesh.ply"), "--mvs",
                          str(tmp_path / "local" / "MVS"), "--image_root", str(tmp_path / "images"), "--out", str(tmp_path / "cli" / "tex.ply")]
                         + lflags + tflags, cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert res.returncode == 0, res.stderr[-3000:]
    print(res.stdout.strip())
    assert "levelled locally" in res.stdout and "levelled locally: 0 seam edges" not in res.stdout
    for name in ["tex.ply"] + files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "local" / name).read_bytes(), name
    # texture_mesh on the files' mesh and views
    mv, mf = mesh.read_ply(str(tmp_path / "local" / "mesh.ply"))
    views = ortho.load_mvs_views(str(tmp_path / "local" / "MVS"), str(tmp_path / "images"))
    tm = texture.texture_mesh(torch.from_numpy(mv).cuda(), torch.from_numpy(mf).cuda(), views, views_per_batch=2, page_size=256,
                              local={"radius": 10, "iterations": 300})
    assert tm["local"]["seam_edges"] > 0
    for name, page in zip(files, tm["pages"]):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "local" / name)).convert("RGB")), page), name
