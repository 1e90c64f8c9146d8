"""The orthophoto of the textured mesh on the GPU (csrc/ortho_mesh.hip om_*, ortho_mesh.mesh_to_ortho): bit-equal to the numpy
restatement of tests/test_ortho_mesh.py on meshes that take the small and the big path, invariant to the face order, winding and
corner rotation, its height the mesh DSM's; on ortho_scene's block it gives back the scene's texture; the pipeline stage, the
command line and predict write the same files for one rank and two."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import test_dsm_mesh as T
import test_ortho_mesh as TM
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _gpu(V, F, tc, tn, words, grid, z_down=False):
    """words: the pages as [h_k, P] uint32 RGBA8 words."""
    from deep3d_aerial_amd import ortho_mesh

    atlas = _cuda(np.concatenate(words, 0).view(np.int32), np.int32)
    rows = _cuda(np.concatenate([[0], np.cumsum([w.shape[0] for w in words])]), np.int64)
    rgba, height = ortho_mesh.mesh_to_ortho(_cuda(V, np.float32).reshape(-1, 3), _cuda(F, np.int32).reshape(-1, 3),
                                            _cuda(tc, np.float32).reshape(-1, 6), _cuda(tn, np.int32).reshape(-1), atlas, rows, grid, z_down)
    return rgba.cpu().numpy(), height.cpu().numpy()


def _pages(words):
    return [np.ascontiguousarray(w).view(np.uint8).reshape(w.shape[0], w.shape[1], 4) for w in words]


def _same(got, want):
    """got (rgba, height) against the restatement's (key, rgba, height)."""
    assert np.array_equal(got[0], want[1]), int((got[0] != want[1]).any(2).sum())
    assert got[1].shape == want[2].shape and np.array_equal(T._bits(got[1]), T._bits(want[2]))


# ----------------------------------------------------------------------------------------
# the random scene: every path of the kernels and every case of the rule
# ----------------------------------------------------------------------------------------
def lattice(nx, ny, seed, spacing=0.5, origin=0.25, jitter=0.3, lift=0.0):
    """A jittered nx x ny height field (test_dsm_mesh.height_field on a rectangle), each quad cut along a random diagonal."""
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(origin + np.arange(nx) * spacing, origin + np.arange(ny) * spacing)
    inner = np.zeros((ny, nx), bool)
    inner[1:-1, 1:-1] = True
    move = inner & (rng.uniform(size=(ny, nx)) < 0.5)
    X = np.where(move, X + rng.uniform(-jitter, jitter, (ny, nx)) * spacing, X)
    Y = np.where(move, Y + rng.uniform(-jitter, jitter, (ny, nx)) * spacing, Y)
    Z = np.sin(X * 0.8) * 1.5 + np.cos(Y * 0.6) + rng.uniform(0, 0.25, (ny, nx)) + lift
    V = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    F = []
    for r in range(ny - 1):
        for c in range(nx - 1):
            a, b, d, e = r * nx + c, r * nx + c + 1, (r + 1) * nx + c + 1, (r + 1) * nx + c
            F += [[a, b, d], [a, d, e]] if rng.uniform() < 0.5 else [[a, b, e], [b, d, e]]
    return V, np.array(F, np.int32)


def random_scene(seed):
    """(V, F, texcoord, texnumber, words, grid): a jittered 40 x 24 height field with about 3 % of its faces flipped and six
    degenerate, a second sheet above a third of the footprint, twenty exactly duplicated faces with other texcoords, four
    triangles whose range exceeds 64 cells (one over the whole raster), 10 % of the faces untextured (equal pairs, non-finite
    texcoords, texnumber out of range); two random RGBA8 pages of width 64 and unequal heights; a 97 x 61 raster with ux != uy
    whose border cuts the mesh (seed 2: with Z bounds that cut it too)."""
    from deep3d_aerial_amd import dsm

    rng = np.random.default_rng(1000 + seed)
    V, F = lattice(40, 24, seed)
    flip = rng.uniform(size=len(F)) < 0.03
    F[flip] = F[flip][:, ::-1]
    deg = rng.choice(len(F), 6, replace=False)
    F[deg[:3], 1] = F[deg[:3], 0]                                            # two equal vertices
    Vd = np.array([[3, 3, 1], [5, 5, 2], [4, 4, 9], [6, 2, 1], [6, 2, 4], [8, 3, 2]], np.float32)   # collinear in xy; vertical
    sheet_v, sheet_f = lattice(14, 24, seed + 7, lift=3.0)                    # x up to 6.75 of 19.75: a third of the footprint
    big_v = np.array([[2, 2, 2.5], [9, 2.5, 3.5], [3, 8, 3],                  # ranges far above 64 cells, cutting through the sheets
                      [10, 1, -1.5], [19, 4, -0.5], [12, 11, -1],
                      [5, 9, 5], [16, 10, 5.5], [15, 3, 4.5],
                      [-30, -20, 0.8], [60, -20, 1.2], [10, 70, 1.0]], np.float32)   # over the whole raster
    V, F = T.merge((V, F), (Vd, [[0, 1, 2], [3, 4, 5]]), (sheet_v, sheet_f), (big_v, np.arange(12).reshape(4, 3)))
    F[deg[3]] = [len(V) - 12, len(V) - 12, len(V) - 12]                      # one vertex three times
    dup = rng.choice(40 * 24, 20, replace=False)
    F = np.concatenate([F, F[dup]])
    m = len(F)
    tc = rng.uniform(0.01, 0.99, (m, 6)).astype(np.float32)
    tc[-4 - 20:-20] = rng.uniform(-0.1, 1.1, (4, 6))                         # the big faces also tap past the pages' edges: the clamp
    tn = rng.integers(0, 2, m).astype(np.int32)
    plain = np.flatnonzero(rng.uniform(size=m) < 0.10)
    kind = rng.integers(0, 4, len(plain))
    tc[plain[kind <= 1]] = np.tile(rng.uniform(0, 1, ((kind <= 1).sum(), 2)).astype(np.float32), (1, 3))   # three equal pairs
    bad = plain[kind == 2]
    tc[bad, rng.integers(0, 6, len(bad))] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), len(bad))
    tn[plain[kind == 3]] = rng.choice(np.int32([-1, 2, 100, -(1 << 31)]), (kind == 3).sum())
    words = [rng.integers(0, 1 << 32, (h, 64), dtype=np.uint64).astype(np.uint32) for h in (48, 31)]
    border = [1.3, 1.3 + 97 * 0.19, 11.27 - 61 * 0.17, 11.27] + ([-1.0, 7.2] if seed == 2 else [])
    return V, F, tc, tn, words, dsm.DsmGrid(border, [0.19, 0.17], size=(97, 61))


_WANT = {}


def _want(seed, z_down):
    """The restatement of the random scene, computed once per (seed, z_down) and shared."""
    if (seed, z_down) not in _WANT:
        V, F, tc, tn, words, g = random_scene(seed)
        _WANT[seed, z_down] = TM.mesh_ortho_numpy(V, F, tc, tn, _pages(words), g, z_down)
    return _WANT[seed, z_down]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("z_down", [False, True])
def test_the_random_scene_is_bit_equal_to_numpy(seed, z_down):
    from deep3d_aerial_amd import dsm

    V, F, tc, tn, words, g = random_scene(seed)
    want = _want(seed, z_down)
    _same(_gpu(V, F, tc, tn, words, g, z_down), want)
    # the scene holds what it says: both paths, untextured tops, coloured and empty cells
    _, _, box = T.triangles(V, F)
    j0, j1, i0, i1, ok = T.cell_ranges(box, g)
    n = (j1 - j0 + 1) * (i1 - i0 + 1)
    assert (ok & (n > dsm.DSM_TRI_SMALL)).sum() >= 4 and (ok & (n <= dsm.DSM_TRI_SMALL)).sum() > 1000
    alpha, covered = want[1][:, :, 3], np.isfinite(want[2])
    assert set(np.unique(alpha)) == {0, 255} and (covered & (alpha == 0)).sum() > 50 and (alpha == 255).sum() > 3000
    assert covered.all() or seed == 2   # the triangle over the whole raster covers every cell the Z bounds leave


def test_face_order_winding_and_corner_rotation_do_not_change_a_bit():
    rng = np.random.default_rng(4)
    V, F, tc, tn, words, g = random_scene(1)
    for z_down in (False, True):
        want = _want(1, z_down)
        p = rng.permutation(len(F))
        _same(_gpu(V, F[p], tc[p], tn[p], words, g, z_down), want)
        Fr, tr = TM.reverse(F, tc)
        _same(_gpu(V, Fr, tr, tn, words, g, z_down), want)
        for r in (1, 2):
            Fr, tr = TM.rotate(F, tc, r)
            _same(_gpu(V, Fr, tr, tn, words, g, z_down), want)
    # the vertex list renumbered
    q = rng.permutation(len(V))
    _same(_gpu(V[q], np.argsort(q)[F].astype(np.int32), tc, tn, words, g), _want(1, False))


def test_the_height_is_the_mesh_dsm():
    from deep3d_aerial_amd import dsm

    for seed in (0, 2):
        V, F, tc, tn, words, g = random_scene(seed)
        h = dsm.mesh_to_dsm(_cuda(V, np.float32), _cuda(F, np.int32), g).cpu().numpy()
        assert np.array_equal(T._bits(_gpu(V, F, tc, tn, words, g)[1]), T._bits(h))
        assert np.array_equal(T._bits(h), T._bits(_want(seed, False)[2]))


@pytest.mark.parametrize("texels_per_cell", [0.125, 8.0])
def test_the_big_path_alone_magnified_and_minified(texels_per_cell):
    """Two textured triangles over a 300 x 200 raster, the page laid over the raster: cells 8 times finer than the texels
    (magnification: neighbouring cells blend the same four texels) and 8 times coarser (minification: one tap per cell, no
    filtering -- the rule's, stated as out of scope)."""
    from deep3d_aerial_amd import dsm

    g = dsm.DsmGrid([0.0, 30.0, 0.0, 20.0], [0.1, 0.1])
    assert g.shape == (200, 300)
    ext = (-0.5, 30.7, -0.3, 20.4)
    V, F = T.quad(ext[0], ext[1], ext[2], ext[3], lambda x, y: 0.1 * x - 0.05 * y + 3.0)
    P, h = int(round(300 * texels_per_cell)), int(round(200 * texels_per_cell))
    rng = np.random.default_rng(int(P))
    words = [rng.integers(0, 1 << 32, (7, P), dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, (h, P), dtype=np.uint64).astype(np.uint32)]
    tc = TM.planar_texcoords(V, F, (0.0, 30.0, 0.0, 20.0))
    tn = np.int32([1, 1])
    for z_down in (False, True):
        want = TM.mesh_ortho_numpy(V, F, tc, tn, _pages(words), g, z_down)
        assert (want[1][:, :, 3] == 255).all()
        _same(_gpu(V, F, tc, tn, words, g, z_down), want)
    # two independent uniform bytes differ by 85 levels on average.  Magnified, neighbouring cells move an eighth of a texel:
    # about 85 / 8; minified, they are blends of different texels: about half of 85.  85 / 4 lies between the two
    step = np.abs(np.diff(want[1][:, :, :3].astype(np.int32), axis=1)).mean()
    assert step < 85 / 4 if texels_per_cell < 1 else step > 85 / 4, step


def test_empty_meshes_and_refusals():
    from deep3d_aerial_amd import dsm, ortho_mesh

    g = T.grid_small()
    words = [np.full((4, 8), 0xff102030, np.uint32)]
    rgba, h = _gpu(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0), words, g)
    assert (rgba == 0).all() and np.isnan(h).all()
    rgba, h = _gpu(np.zeros((5, 3)), np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0), words, g, True)
    assert (rgba == 0).all() and np.isnan(h).all()
    ok = {k: v.cuda() for k, v in TM._cpu_inputs().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, atlas=ok["atlas"].cpu()))
    with pytest.raises(ValueError, match="outside"):
        ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, faces=ok["faces"] + 2))
    with pytest.raises(ValueError, match="rise"):
        ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, page_row=torch.tensor([0, 6, 9]).cuda()))
    rgba, h = ortho_mesh.mesh_to_ortho(grid=g, **ok)   # four vertices at the origin: degenerate faces, nothing covered
    assert int(rgba.sum()) == 0 and bool(torch.isnan(h).all())


# ----------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------
def test_the_scene_rendered_from_its_textured_mesh_gives_back_its_texture():
    """ortho_scene's block, meshed and textured as in test_texture_gpu.test_the_textured_scene_gives_back_its_texture, rendered
    with z_down (its cameras are on the low-Z side) on a 0.25 m grid over scene_border.  On the cells with alpha 255 the error
    against OS.texture at the cell centre (largest channel) meets that test's bounds -- median <= 10 levels, 90 % within 20: the
    mesh lies within a voxel (0.4 m) of the surface and the texture changes by up to 33 levels per metre.  The raster flipped
    left-right errs at least 3 times as much in the median.  The coloured cells number at least 90 % of the cells
    ortho.dsm_to_ortho colours on the DSM mesh_to_dsm gives for the same grid."""
    import test_texture_gpu as TG
    from deep3d_aerial_amd import dsm, mesh, ortho, ortho_mesh, texture

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    mviews = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda())
              for v in scene.views]
    v, f = mesh.depth_to_mesh(mviews, mesh.MeshGrid(border, voxel))
    ov = TG._views([dict(s, id=i) for i, s in enumerate(scene.views)])
    res = texture.texture_mesh(v, f, ov, page_size=256)
    atlas, rows = ortho_mesh.atlas_from_pages(res["pages"], 256, "cuda")
    g = dsm.DsmGrid(border[:4], [0.25, 0.25])
    rgba, height = ortho_mesh.mesh_to_ortho(v, f, res["texcoord"], res["texnumber"], atlas, rows, g, z_down=True)
    s = ortho_mesh.summary(rgba, height)
    rgba = rgba.cpu().numpy()
    X, Y = np.meshgrid(g.x_min + (np.arange(g.width) + 0.5) * g.unit[0], g.y_max - (np.arange(g.height) + 0.5) * g.unit[1])
    on = rgba[:, :, 3] == 255
    assert on.sum() == s["coloured"] and s["coloured"] + s["untextured"] + s["empty"] == g.width * g.height
    want = OS.texture(X, Y)
    err = np.abs(rgba[:, :, :3].astype(np.float64) - want).max(2)[on]
    flipped = rgba[:, ::-1]
    fon = on & (flipped[:, :, 3] == 255)
    ctrl = np.abs(flipped[:, :, :3].astype(np.float64) - want).max(2)[fon]
    draped, view, _ = ortho.dsm_to_ortho(dsm.mesh_to_dsm(v, f, g), g, ov)
    n_draped = int((view >= 0).sum())
    print("mesh orthophoto: %d x %d cells, %d coloured, %d untextured, %d empty; error median %.2f, 90th percentile %.2f, max %.2f "
          "levels; flipped control median %.2f over %d cells; ortho.dsm_to_ortho colours %d cells"
          % (g.width, g.height, s["coloured"], s["untextured"], s["empty"], np.median(err), np.percentile(err, 90), err.max(),
             np.median(ctrl), int(fon.sum()), n_draped))
    assert s["coloured"] > 1000
    assert np.median(err) <= 10.0 and np.percentile(err, 90) <= 20.0
    assert np.median(ctrl) >= 3 * np.median(err)
    assert s["coloured"] >= 0.9 * n_draped


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _launch(n_ranks, script, out_dir, border, voxel, *extra):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", script), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel)] + [repr(e) for e in extra]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def _listing(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(folder) for f in fs)


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The scene through predict_and_fuse with the "ortho" key on one rank, launched once: (folder, stdout, border, voxel)."""
    border, voxel = TS.scene_border(OS.ImageSceneViews())
    folder = tmp_path_factory.mktemp("ortho_mesh") / "one"
    return folder, _launch(1, "ortho_mesh_scene.py", folder, border, voxel, 0.25), border, voxel


def test_one_and_two_ranks_and_the_command_line_write_the_same_orthophoto(tmp_path, one_rank):
    from deep3d_aerial_amd import dsm, ortho_mesh, texture

    one, out1, border, voxel = one_rank
    out2 = _launch(2, "ortho_mesh_scene.py", tmp_path / "two", border, voxel, 0.25)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2 and "ortho -" in out2
    for name in ("ortho.tif", "ortho.tfw", "tex.ply", "mesh.ply"):
        assert (one / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    g = dsm.DsmGrid(border[:4], [0.25, 0.25])
    assert (one / "ortho.tfw").read_text() == g.tfw_text()
    # the command line on the written PLY and pages
    cli = tmp_path / "cli" / "o.tif"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.ortho_mesh", "--textured", str(one / "tex.ply"), "--out", str(cli),
           "--border=%s" % ",".join(repr(b) for b in border[:4]), "--unit=0.25", "--z_down"]
    res = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == (one / "ortho.tif").read_bytes()
    assert (tmp_path / "cli" / "o.tfw").read_text() == g.tfw_text()
    assert "cells coloured" in res.stdout
    # the file holds the operator's raster of the written mesh
    V, F, tc, tn, files = texture.read_textured_ply(str(one / "tex.ply"))
    pages = ortho_mesh.read_pages(str(one / "tex.ply"), files)
    atlas, rows = ortho_mesh.atlas_from_pages(pages, pages[0].shape[1], "cuda")
    rgba, _ = ortho_mesh.mesh_to_ortho(_cuda(V, np.float32), _cuda(F, np.int32), _cuda(tc, np.float32), _cuda(tn, np.int32), atlas, rows, g, True)
    from deep3d_aerial_amd import ortho

    assert ortho.tiff_bytes(rgba.cpu().numpy(), g) == cli.read_bytes() and int((rgba[:, :, 3] == 255).sum()) > 1000


def test_without_the_ortho_key_the_folder_lists_what_it_lists_today(tmp_path, one_rank):
    with_dir, _, border, voxel = one_rank
    _launch(1, "texture_scene.py", tmp_path / "plain", border, voxel)     # the texture stage as it was: no "ortho" key
    plain, with_ = _listing(tmp_path / "plain"), _listing(with_dir)
    assert "ortho.tif" not in plain and not [f for f in plain if f.endswith((".tif", ".tfw"))]
    assert sorted(plain + ["ortho.tif", "ortho.tfw"]) == with_
    for name in (f for f in plain if not f.startswith("MVS")):   # the mesh, the textured mesh and its pages
        assert (tmp_path / "plain" / name).read_bytes() == (with_dir / name).read_bytes(), name


def test_predict_main_fuse_mesh_texture_and_texture_ortho(tmp_path):
    """predict --fuse --mesh --texture --texture_ortho on the block fixture (seeded casmvsnet weights: plumbing, not geometry):
    the orthophoto is written on the mesh's footprint at the default unit, and the command line gives the same file."""
    import block_fixture as BF
    from deep3d_aerial_amd import dsm, mvs_dl, predict as P, synthetic as S

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    S.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    ply, tex, tif = tmp_path / "mesh" / "block.ply", tmp_path / "tex" / "block.ply", tmp_path / "tex" / "block_ortho.tif"
    flags = ["--border=-200,400,-200,200,-600,100", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    tflags = ["--depth_tolerance=0.5", "--page_size=256", "--views_per_batch=2"]
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                     "--position_threshold=50", "--mesh", str(ply)] + ["--mesh_" + f[2:] for f in flags] +
                         ["--texture", str(tex)] + ["--texture_" + f[2:] for f in tflags] +
                         ["--texture_ortho", str(tif), "--texture_ortho_unit=5"]).run(folder, str(tmp_path / "MVS"))
    assert tif.exists() and tex.exists()
    g = dsm.DsmGrid([-200.0, 400.0, -200.0, 200.0], [5.0, 5.0])
    assert (tmp_path / "tex" / "block_ortho.tfw").read_text() == g.tfw_text()
    cli = tmp_path / "cli" / "o.tif"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.ortho_mesh", "--textured", str(tex), "--out", str(cli),
                          "--border=-200,400,-200,200", "--unit=5"], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == tif.read_bytes()
