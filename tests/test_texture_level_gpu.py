"""The seam levelling kernels (csrc/texture_level.hip) on the GPU: nodes, seam pairs, smoothness edges, CSR, samples and
right-hand side bit-equal to the numpy restatement of tests/test_texture_level.py; the conjugate gradients against the dense fp64
solve; the coverage keys and the levelled pages bit-equal given the same g; a scene whose views differ in gain and offset; and
the option through texture_mesh, the pipeline on one and two ranks, predict and the standalone command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import pipeline_scene as PS
import test_texture as T
import test_texture_gpu as G
import test_texture_level as L
import texture_scene as TS

ROOT = G.ROOT
pytestmark = pytest.mark.gpu
SOLVE_TOLERANCE = 1e-6   # of the solve test: the restatement then lies 0.0035 and 0.0043 levels from the dense solve (<= 0.05 / 4)


@functools.lru_cache(maxsize=None)
def _reference(seed, n, n_views, page_size=256):
    """A random scene of test_texture_gpu with its first n_views views and the restatement's results (dense solve); shared and
    never changed."""
    V, F, vs = G._random_scene(seed, n)
    vs = vs[:n_views]
    key = T.select_numpy(V, F, vs)
    return V, F, vs, key, L.level_numpy(V, F, key, vs, page_size)


def _gpu_layout(V, F, vs, page_size=256):
    """The GPU's keys, layout and filled (not finished) atlas of a scene."""
    from deep3d_aerial_amd import texture

    v, f = G._mesh(V, F)
    ov = G._views(vs)
    key = texture.select_faces(v, f, ov)
    chart, labels, rects, packing, table = texture.layout(v, f, key, ov, page_size)
    atlas = texture.fill_pages(table, packing, ov, texture.new_atlas(packing, v.device))
    return v, f, ov, key, chart, packing, table, atlas


def _rgb(atlas):
    return atlas.contiguous().view(torch.uint8).reshape(atlas.shape[0], atlas.shape[1], 4)[:, :, :3].cpu().numpy()


def _check_graph(graph, want):
    assert np.array_equal(graph.nodes.cpu().numpy(), want["nodes"])
    assert np.array_equal(graph.face_nodes.cpu().numpy(), want["face_nodes"])
    assert np.array_equal(graph.seams.cpu().numpy(), want["seams"])
    assert np.array_equal(graph.smooth.cpu().numpy(), want["smooth"])
    assert np.array_equal(graph.row_ptr.cpu().numpy(), want["row_ptr"])
    assert np.array_equal(graph.column.cpu().numpy(), want["column"])
    assert np.array_equal(graph.weight.cpu().numpy().view(np.uint32), want["weight"].view(np.uint32))


SCENES = [(0, 16, 3), (1, 24, 4), (3, 24, 2)]


@pytest.mark.parametrize("seed,n,n_views", SCENES)
def test_graph_and_samples_are_bit_equal_to_numpy(seed, n, n_views):
    from deep3d_aerial_amd import texture

    V, F, vs, key, want = _reference(seed, n, n_views)
    gw = want["graph"]
    per_vertex = np.bincount(gw["nodes"] % gw["n"])
    assert len(gw["seams"]) >= 1 and (per_vertex >= 3).any() and 40 <= len(V) <= 400 and len(gw["nodes"]) <= 1500
    if n == 24:
        assert len(gw["nodes"]) > 256 and len(gw["nodes"]) % 64
    v, f, ov, gkey, chart, packing, table, atlas = _gpu_layout(V, F, vs)
    assert np.array_equal(gkey.cpu().numpy(), key) and np.array_equal(chart.cpu().numpy(), want["chart"])
    graph = texture.level_graph(f, chart, len(V))
    _check_graph(graph, gw)
    fg, bg = texture.level_samples(v, graph, table, packing, ov, atlas)
    assert np.array_equal(fg.cpu().numpy()[:, :3].view(np.uint32), want["f"].view(np.uint32))
    assert np.array_equal(bg.cpu().numpy()[:, :3].view(np.uint32), want["b"].view(np.uint32))
    assert not fg[:, 3].any() and not bg[:, 3].any() and want["b"].any()


def test_graph_of_an_empty_mesh_and_of_a_mesh_without_winners():
    from deep3d_aerial_amd import texture

    V, F, vs = G._random_scene(0, 8)
    v, f = G._mesh(V, F)
    for faces, chart in ((f[:0], torch.zeros((0,), dtype=torch.int32, device="cuda")),
                         (f, torch.full((len(F),), -1, dtype=torch.int32, device="cuda"))):
        graph = texture.level_graph(faces, chart, len(V))
        _check_graph(graph, L.level_graph_numpy(faces.cpu().numpy(), chart.cpu().numpy(), len(V)))
        assert graph.n_nodes == 0 and graph.row_ptr.cpu().tolist() == [0]
        g, it, ok = texture.level_solve(graph, torch.zeros((0, 4), device="cuda"))
        assert g.shape == (0, 4) and it == 0 and ok
    # no winners through the whole chain: nothing to level, the pages stay
    far = [dict(x, E=np.float32(np.eye(4)) + np.float32([[0, 0, 0, 1e4], [0] * 4, [0] * 4, [0] * 4])) for x in vs[:2]]
    res = texture.texture_mesh(v, f, G._views(far), page_size=256, level={})
    assert res["level"]["nodes"] == 0 and res["packing"].heights == [2]


@pytest.mark.parametrize("seed,n,n_views", SCENES[1:])
def test_solve_against_the_dense_solve(seed, n, n_views):
    """g of the GPU against the dense fp64 solution, in grey levels (max over nodes and channels).  The numpy restatement of the
    iteration (the same fp32 vectors, fp64 dots and stop rule, tolerance 1e-6) lies 0.0035 (seed 1, 470 nodes) and 0.0043 (seed 3, 465 nodes) from it;
    the GPU, whose dot products are summed in another order, is allowed four times that, which must stay <= 0.05."""
    from deep3d_aerial_amd import texture

    V, F, vs, key, want = _reference(seed, n, n_views)
    gw = want["graph"]
    rest, it_rest, ok_rest = L.cg_numpy(gw, want["b"], tolerance=SOLVE_TOLERANCE, iterations=500)
    allowed = 4 * np.abs(rest - want["g"]).max()
    assert ok_rest and allowed <= 0.05
    v, f, ov, gkey, chart, packing, table, atlas = _gpu_layout(V, F, vs)
    graph = texture.level_graph(f, chart, len(V))
    _, b = texture.level_samples(v, graph, table, packing, ov, atlas)
    g, it, ok = texture.level_solve(graph, b, tolerance=SOLVE_TOLERANCE, iterations=500)
    dist = np.abs(g.cpu().numpy()[:, :3].astype(np.float64) - want["g"]).max()
    print("solve: restatement %.5f levels in %d iterations, GPU %.5f in %d, allowed %.5f" % (allowed / 4, it_rest, dist, it, allowed))
    assert ok and it < 500   # the tolerance stopped it, not the cap
    assert dist <= allowed
    assert not g[:, 3].any()
    # the cap: one iteration is not enough
    g1, it1, ok1 = texture.level_solve(graph, b, tolerance=SOLVE_TOLERANCE, iterations=17)
    assert it1 == 17 and not ok1
    # two runs give the same bits
    g2, it2, _ = texture.level_solve(graph, b, tolerance=SOLVE_TOLERANCE, iterations=500)
    assert it2 == it and torch.equal(g2, g)


@pytest.mark.parametrize("seed,n,n_views", SCENES)
def test_coverage_and_apply_are_bit_equal_given_the_same_g(seed, n, n_views):
    from deep3d_aerial_amd import texture

    V, F, vs, key, want = _reference(seed, n, n_views)
    v, f, ov, gkey, chart, packing, table, atlas = _gpu_layout(V, F, vs)
    graph = texture.level_graph(f, chart, len(V))
    cover = texture.level_coverage(v, f, chart, table, packing, ov)
    assert np.array_equal(cover.cpu().numpy(), want["cover"]) and (want["cover"] != L.EMPTY).sum() > 500
    g = torch.zeros((graph.n_nodes, 4), dtype=torch.float32, device="cuda")
    g[:, :3] = torch.from_numpy(want["g"].astype(np.float32)).cuda()
    alpha = atlas.clone() & -16777216   # 0xff000000 as int32
    texture.level_apply(v, f, chart, graph, g, cover, table, packing, ov, atlas)
    assert torch.equal(atlas & -16777216, alpha)
    got = _rgb(texture.finish_pages(atlas))
    assert np.array_equal(got, want["levelled"]) and (got != want["atlas"]).any()


# ----------------------------------------------------------------------------------------
# a scene whose views differ in gain and offset
# ----------------------------------------------------------------------------------------
GAINS = [(1.00, 0), (0.80, 30), (1.15, -25), (0.90, -30), (1.10, 25), (0.85, 20), (1.20, -20)]


@functools.lru_cache(maxsize=None)
def _gain_scene():
    """texture_scene's scene (ortho_scene's views and rendered images), every image through its own gain and offset, and a mesh
    of 20 x 15 vertices: a pixel grid of view 0's depth map, back-projected."""
    scene = OS.ImageSceneViews()
    vs = []
    for i, (s, (gain, offset)) in enumerate(zip(scene.views, GAINS)):
        img = np.clip(np.rint(s["image"].astype(np.float64) * gain + offset), 0, 255).astype(np.uint8)
        vs.append({"id": i, "K": s["K"], "E": s["E"], "depth": s["depth"], "image": img})
    v0 = scene.views[0]
    K, E = v0["K"].astype(np.float64), v0["E"].astype(np.float64)
    R, t = E[:3, :3], E[:3, 3]
    xs, ys = np.rint(np.linspace(3, scene.w - 4, 20)).astype(int), np.rint(np.linspace(3, scene.h - 4, 15)).astype(int)
    X, Y = np.meshgrid(xs, ys)
    d = v0["depth"][Y.ravel(), X.ravel()].astype(np.float64)
    rays = np.linalg.inv(K) @ np.stack([X.ravel(), Y.ravel(), np.ones(X.size)])
    V = (R.T @ (rays * d - t[:, None])).T.astype(np.float32)
    F = []
    ny, nx = X.shape
    for i in range(ny - 1):
        for j in range(nx - 1):
            a, b, c, e = i * nx + j, i * nx + j + 1, (i + 1) * nx + j, (i + 1) * nx + j + 1
            F += [[a, c, b], [b, c, e]]
    return V, np.array(F, np.int32), vs


def _steps(V, vs, res, atlas, levelled):
    before = L.seam_step(res["graph"], L.level_samples_numpy(V, res["graph"], res["rects"], res["packing"], res["ids"], vs, atlas))
    after = L.seam_step(res["graph"], L.level_samples_numpy(V, res["graph"], res["rects"], res["packing"], res["ids"], vs, levelled))
    return before, after


@functools.lru_cache(maxsize=None)
def _gain_reference():
    V, F, vs = _gain_scene()
    key = T.select_numpy(V, F, vs)
    res = L.level_numpy(V, F, key, vs, 256)
    return key, res, _steps(V, vs, res, res["atlas"], res["levelled"])


def test_levelling_evens_out_gain_and_offset_end_to_end():
    """The mean absolute difference of the two sides' taps over all seam pairs, from the pages: the restatement's drops below
    half (the condition), and the GPU's after lies within one level of the restatement's."""
    from deep3d_aerial_amd import texture

    V, F, vs = _gain_scene()
    key, want, (before, after) = _gain_reference()
    assert len(want["graph"]["seams"]) > 10 and len(want["labels"]) >= 3
    assert after < 0.5 * before
    v, f = G._mesh(V, F)
    plain = texture.texture_mesh(v, f, G._views(vs), page_size=256)
    res = texture.texture_mesh(v, f, G._views(vs), page_size=256, level={})
    assert np.array_equal(res["key"].cpu().numpy(), key) and res["level"]["converged"] and res["level"]["seams"] == len(want["graph"]["seams"])
    assert np.array_equal(L.stack_pages(plain["pages"]), want["atlas"])
    g_before, g_after = _steps(V, vs, want, L.stack_pages(plain["pages"]), L.stack_pages(res["pages"]))
    print("seam step: before %.2f, after %.2f (numpy), %.2f (GPU), %d iterations" % (before, after, g_after, res["level"]["iterations"]))
    assert g_before == before and abs(g_after - after) <= 1.0
    assert torch.equal(res["texcoord"], plain["texcoord"]) and torch.equal(res["texnumber"], plain["texnumber"])


def test_one_view_only_and_off_by_default():
    from deep3d_aerial_amd import texture

    V, F, vs = _gain_scene()
    v, f = G._mesh(V, F)
    one = texture.texture_mesh(v, f, G._views(vs[:1]), page_size=256)
    lev = texture.texture_mesh(v, f, G._views(vs[:1]), page_size=256, level={})
    assert len(one["labels"]) >= 1 and lev["level"]["nodes"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(one["pages"], lev["pages"]))
    # level=None is today's call: the same result, bit for bit, and no "level" entry
    a = texture.texture_mesh(v, f, G._views(vs), 0.01, None, 256, 2, texture.EMPTY_COLOR)
    b = texture.texture_mesh(v, f, G._views(vs), 0.01, None, 256, 2, texture.EMPTY_COLOR, level=None)
    assert "level" not in b and set(a) == set(b)
    assert torch.equal(a["key"], b["key"]) and torch.equal(a["texcoord"], b["texcoord"]) and torch.equal(a["texnumber"], b["texnumber"])
    assert all(np.array_equal(x, y) for x, y in zip(a["pages"], b["pages"]))
    want = T.texture_numpy(V, F, vs, 0.01, 256)
    assert all(np.array_equal(x, y) for x, y in zip(b["pages"], want["pages"]))


def test_two_runs_view_order_and_batching_give_the_same_levelled_pages():
    from deep3d_aerial_amd import texture

    V, F, vs = _gain_scene()
    v, f = G._mesh(V, F)
    first = None
    for vpb, order in ((None, vs), (None, vs), (2, vs[::-1]), (3, [vs[i] for i in (3, 0, 6, 1, 2, 5, 4)])):
        res = texture.texture_mesh(v, f, G._views(order), views_per_batch=vpb, page_size=256, level={"tolerance": 1e-5})
        pages = L.stack_pages(res["pages"])
        first = pages if first is None else first
        assert np.array_equal(pages, first)


def test_level_inputs_are_checked():
    from deep3d_aerial_amd import texture

    V, F, vs, key, want = _reference(0, 16, 3)
    v, f, ov, gkey, chart, packing, table, atlas = _gpu_layout(V, F, vs)
    args = lambda a: (v, f, gkey, chart, table, packing, ov, a)
    with pytest.raises(ValueError):
        texture.level_pages(*args(atlas[:-1]))
    with pytest.raises(ValueError):
        texture.level_pages(*args(atlas.to(torch.int64)))
    with pytest.raises(RuntimeError):
        texture.level_pages(*args(atlas.cpu()))
    with pytest.raises(RuntimeError):
        texture.level_pages(v.cpu(), f.cpu(), gkey.cpu(), chart.cpu(), table, packing, ov, atlas)
    with pytest.raises(RuntimeError):
        texture.level_graph(f.cpu(), chart.cpu(), len(V))
    for bad in ({"smooth": -1.0}, {"anchor": 0.0}, {"tolerance": 1.0}, {"iterations": 0}):
        with pytest.raises(ValueError):
            texture.level_pages(*args(atlas), **bad)
        with pytest.raises(ValueError):
            texture.texture_mesh(v, f, ov, page_size=256, level=bad)


# ----------------------------------------------------------------------------------------
# the pipeline stage and the command lines
# ----------------------------------------------------------------------------------------
LEVEL_SCENE = """import os, sys
sys.path[:0] = [%r, %r]
import numpy as np
import texture_scene as TS
import test_texture_level_gpu as LG

init = TS.OS.ImageSceneViews.__init__


def gained(self, *args, **kwargs):   # every image through its own gain and offset
    init(self, *args, **kwargs)
    for v, (gain, offset) in zip(self.views, LG.GAINS):
        v["image"] = np.clip(np.rint(v["image"].astype(np.float64) * gain + offset), 0, 255).astype(np.uint8)


TS.OS.ImageSceneViews.__init__ = gained
level = {} if sys.argv[4] == "1" else None
settings = TS.texture_settings
TS.texture_settings = lambda path, **kw: dict(settings(path, **kw), level=level)
TS.main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]))
"""


def _launch(n_ranks, out_dir, border, voxel, script, level):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script), str(out_dir), ",".join(repr(b) for b in border), repr(voxel), "1" if level else "0"]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_levelled_mesh_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import texture

    script = tmp_path / "level_scene.py"
    script.write_text(LEVEL_SCENE % (ROOT, os.path.join(ROOT, "tests")))
    border, voxel = TS.scene_border(OS.ImageSceneViews())
    _launch(1, tmp_path / "one", border, voxel, script, True)
    _launch(2, tmp_path / "two", border, voxel, script, True)
    _, _, _, _, files = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    for name in ["tex.ply", "mesh.ply"] + files:
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    # the standalone command on the mesh and MVS folder the stage wrote, the images as files: --level writes the stage's files,
    # without it the same PLY (levelling moves no texcoord) and other pages
    from PIL import Image

    V, F, vs = _gain_scene()
    for i, v in enumerate(vs):
        (tmp_path / "images").mkdir(exist_ok=True)
        Image.fromarray(v["image"]).save(str(tmp_path / "images" / ("scene_%02d.png" % i)))
    for what, extra in (("cli", ["--level"]), ("plain", [])):
        res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.texture", "--mesh", str(tmp_path / "one" / "mesh.ply"), "--mvs",
                              str(tmp_path / "one" / "MVS"), "--image_root", str(tmp_path / "images"), "--out", str(tmp_path / what / "tex.ply"),
                              "--page_size=256"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
        assert res.returncode == 0, res.stderr[-3000:]
        print(res.stdout.strip())
    for name in ["tex.ply"] + files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "one" / name).read_bytes(), name
    assert (tmp_path / "plain" / "tex.ply").read_bytes() == (tmp_path / "one" / "tex.ply").read_bytes()
    assert any((tmp_path / "plain" / name).read_bytes() != (tmp_path / "one" / name).read_bytes() for name in files)


def test_predict_main_texture_level_and_the_standalone_level_flag(tmp_path, monkeypatch):
    """predict.main --fuse --mesh --texture, with and without --texture_level, on the gain and offset scene, and
    python -m deep3d_aerial_amd.texture --level on the mesh and MVS folder it wrote.  The scene enters predict.main the way it
    enters the pipeline tests: pipeline_scene's dataset stands for --synthetic_items' block and its SceneModel (the rendered
    depth maps) for the network, since seeded weights reconstruct no surface; the argument parsing, the settings, the stages
    and the files are predict's own.  The mesh has faces and seams: the pages predict writes with the flag differ from those
    without it (this fails when predict drops the flag), the PLY bytes are the same (levelling moves no texcoord), and the
    standalone --level writes the flag's files."""
    from PIL import Image
    from deep3d_aerial_amd import predict as P, texture

    scene = OS.ImageSceneViews()
    for v, (gain, offset) in zip(scene.views, GAINS):
        v["image"] = np.clip(np.rint(v["image"].astype(np.float64) * gain + offset), 0, 255).astype(np.uint8)
    monkeypatch.setattr(P, "SyntheticBlock", lambda *a, **k: scene)
    monkeypatch.setattr(P, "build_model", lambda *a, **k: PS.SceneModel(scene))
    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    border, voxel = TS.scene_border(scene)
    tflags = ["--depth_tolerance=0.01", "--page_size=256", "--views_per_batch=2"]

    def run(out, extra):
        P.main(["--synthetic_items", str(len(scene)), "--output_folder", str(out / "MVS"), "--display", "False", "--fuse",
                "--fuse_filter_sources=0", "--fusion_num", str(PS.FUSION_NUM), "--geo_consist_num=3", "--position_threshold=1.0",
                "--depth_threshold=0.01", "--normal_threshold=10.0", "--photometric_threshold=0.2", "--mesh", str(out / "mesh.ply"),
                "--mesh_border=" + ",".join(repr(b) for b in border), "--mesh_voxel=" + repr(voxel), "--mesh_min_views=2",
                "--mesh_conf_threshold=0.2", "--texture", str(out / "tex.ply")] + ["--texture_" + f[2:] for f in tflags] + extra)
        return texture.read_textured_ply(str(out / "tex.ply"))

    _, F, _, _, files = run(tmp_path / "level", ["--texture_level"])
    _, Fp, _, _, files_plain = run(tmp_path / "plain", [])
    assert len(F) > 100 and files and files == files_plain
    # levelling moves no texcoord: the same PLY bytes, other pages
    assert (tmp_path / "plain" / "tex.ply").read_bytes() == (tmp_path / "level" / "tex.ply").read_bytes()
    differ = [name for name in files if (tmp_path / "plain" / name).read_bytes() != (tmp_path / "level" / name).read_bytes()]
    assert differ
    # the standalone command on predict's mesh and MVS folder, the images as files
    (tmp_path / "images").mkdir()
    for i, v in enumerate(scene.views):
        Image.fromarray(v["image"]).save(str(tmp_path / "images" / ("scene_%02d.png" % i)))
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.texture", "--mesh", str(tmp_path / "level" / "mesh.ply"), "--mvs",
                          str(tmp_path / "level" / "MVS"), "--image_root", str(tmp_path / "images"), "--out", str(tmp_path / "cli" / "tex.ply"),
                          "--level"] + tflags, cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert res.returncode == 0, res.stderr[-3000:]
    print(res.stdout.strip())
    assert "levelled" in res.stdout and "levelled 0 seam pairs" not in res.stdout
    for name in ["tex.ply"] + files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "level" / name).read_bytes(), name
