"""The texturing kernels (csrc/texture.hip) and the texture stage of the pipeline on the GPU: keys, charts, rects, pages and
texcoords bit-equal to the numpy restatement of tests/test_texture.py on random meshes and views, independence of batching, view
order and face order, a textured scene whose atlas gives back its texture, and the files written by predict_and_fuse(texture=...)
on one and two ranks, by predict --fuse --mesh --texture and by python -m deep3d_aerial_amd.texture."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import pipeline_scene as PS
import test_ortho as TO
import test_texture as T
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _views(vs):
    from deep3d_aerial_amd import ortho

    return [ortho.OrthoView(v["id"], v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["image"]).cuda())
            for v in vs]


def _mesh(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F, np.int32)).cuda()


def _random_scene(seed, n=40):
    """A height-field mesh of ground (z = 100) and two boxes seen from cameras near z = 0 (test_ortho's world), its vertices
    jittered, with a few flipped and degenerate faces; views of different sizes, some tilted, some reaching past the mesh, depth
    maps perturbed with holes (0 and NaN), and a twin view for exact ties."""
    rng = np.random.default_rng(seed)
    boxes = [(-5.0, 5.0, -6.0, 6.0, 80.0), (12.0, 20.0, 2.0, 9.0, 88.0)]
    xs, ys = np.linspace(-30, 30, n), np.linspace(-18, 18, n * 3 // 5)
    X, Y = np.meshgrid(xs, ys)
    Z = np.full(X.shape, TO.GROUND)
    for x0, x1, y0, y1, top in boxes:
        Z[(X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)] = top
    V = np.stack([X, Y, Z], -1).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (X.size, 3))
    F = []
    ny, nx = X.shape
    for i in range(ny - 1):
        for j in range(nx - 1):
            a, b, c, d = i * nx + j, i * nx + j + 1, (i + 1) * nx + j, (i + 1) * nx + j + 1
            F += [[a, c, b], [b, c, d]]   # normals toward -Z, the cameras
    F = np.array(F, np.int32)
    flip = rng.uniform(size=len(F)) < 0.03
    F[flip] = F[flip][:, ::-1]
    deg = rng.choice(len(F), 6, replace=False)
    F[deg[:3], 2] = F[deg[:3], 0]   # degenerate: a repeated index
    F[deg[3:], 1] = F[deg[3:], 0]
    vs = []
    for k in range(7):
        w, hh = int(rng.integers(60, 200)), int(rng.integers(50, 150))
        C = (rng.uniform(-40, 40), rng.uniform(-25, 25), rng.uniform(0.0, 2.0))
        tilt = (0.0, 0.0) if k % 3 == 0 else (rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4))
        v = TO.view(int(rng.integers(0, 1 << 30)), C, boxes, w=w, h=hh, f=rng.uniform(60, 140), tilt=tilt)
        d = v["depth"] * rng.uniform(0.995, 1.005, v["depth"].shape).astype(np.float32)
        d[rng.uniform(size=d.shape) < 0.03] = 0.0
        d[rng.uniform(size=d.shape) < 0.01] = np.nan
        v["depth"] = d.astype(np.float32)
        vs.append(v)
    vs.append(dict(vs[0], id=vs[0]["id"] ^ 1))
    return V.astype(np.float32), F, vs


def _check_equal(got, want):
    assert np.array_equal(got["key"].cpu().numpy(), want["key"])
    assert np.array_equal(got["chart"].cpu().numpy(), want["chart"])
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    assert np.array_equal(got["rects"].cpu().numpy(), want["rects"])
    assert np.array_equal(got["packing"].place, want["packing"].place) and got["packing"].heights == want["packing"].heights
    assert len(got["pages"]) == len(want["pages"])
    for a, b in zip(got["pages"], want["pages"]):
        assert np.array_equal(a, b)
    assert np.array_equal(got["texcoord"].cpu().numpy().view(np.uint32), want["texcoord"].view(np.uint32))
    assert np.array_equal(got["texnumber"].cpu().numpy(), want["texnumber"])


@pytest.mark.parametrize("seed,page_size,tol", [(0, 256, 0.01), (1, 200, 0.01), (2, 1024, 0.05)])
def test_bit_equal_to_numpy_on_random_meshes(seed, page_size, tol):
    from deep3d_aerial_amd import texture

    V, F, vs = _random_scene(seed)
    want = T.texture_numpy(V, F, vs, tol, page_size)
    got = texture.texture_mesh(*_mesh(V, F), _views(vs), tol, page_size=page_size)
    _check_equal(got, want)
    seen = want["key"] != T.EMPTY
    assert seen.mean() > 0.5 and len(want["labels"]) > 5 and len(set((want["key"][seen] & 0xffffffff).tolist())) > 3
    assert got["packing"].n_pages >= 1


def test_batching_view_order_and_face_order_do_not_change_the_result(tmp_path):
    from deep3d_aerial_amd import texture

    V, F, vs = _random_scene(3)
    v, f = _mesh(V, F)
    files = []
    for k, (vpb, order) in enumerate([(None, vs), (1, vs), (3, vs), (None, vs[::-1]), (2, [vs[i] for i in (3, 0, 6, 1, 7, 2, 5, 4)])]):
        res = texture.texture_mesh(v, f, _views(order), views_per_batch=vpb, page_size=256)
        texture.write_textured_ply(str(tmp_path / ("m%d.ply" % k)), v, f, res["texcoord"], res["texnumber"], res["pages"])
        files.append([(tmp_path / ("m%d.ply" % k)).read_bytes()] + [(tmp_path / ("m%d_%d.png" % (k, p))).read_bytes()
                                                                   for p in range(len(res["pages"]))])
        files[-1][0] = files[-1][0].replace(b"m%d_" % k, b"m_")
        if k == 0:
            key0 = res["key"].cpu().numpy()
        assert np.array_equal(res["key"].cpu().numpy(), key0)
    assert all(fl == files[0] for fl in files[1:])
    # a shuffled face list: the same key per face
    perm = np.random.default_rng(0).permutation(len(F))
    key = texture.select_faces(v, torch.from_numpy(F[perm]).cuda(), _views(vs))
    assert np.array_equal(key.cpu().numpy(), key0[perm])


def test_keys_merged_over_ranks_and_pages_filled_per_rank():
    """What the pipeline does with two ranks, in one process: keys of two view sets merged by a minimum, pages filled per set
    and summed as int32 texels, then the empty colour."""
    from deep3d_aerial_amd import texture

    V, F, vs = _random_scene(4)
    v, f = _mesh(V, F)
    ov = _views(vs)
    whole = texture.texture_mesh(v, f, ov, page_size=256)
    k0 = texture.select_faces(v, f, ov[:3])
    k1 = texture.select_faces(v, f, ov[3:])
    key = torch.minimum(k0, k1)
    assert torch.equal(key, whole["key"])
    cams = [texture.Camera(x.id, x.K, np.vstack([np.hstack([x.R, x.t[:, None]]), [[0, 0, 0, 1]]]), x.W, x.H) for x in ov]
    chart, labels, rects, packing, table = texture.layout(v, f, key, cams, 256)
    a0 = texture.fill_pages(table, packing, ov[:3])
    a1 = texture.fill_pages(table, packing, ov[3:])
    atlas = texture.finish_pages(a0 + a1)
    pages = texture.split_pages(atlas, packing)
    assert all(np.array_equal(a, b) for a, b in zip(pages, whole["pages"]))
    tc, tn = texture.texcoords(v, f, key, chart, table, packing, cams)
    assert torch.equal(tc, whole["texcoord"]) and torch.equal(tn, whole["texnumber"])


def _bilinear(page, x, y):
    H, W = page.shape[:2]
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    p = page.astype(np.float64)
    cl = lambda a, n: np.clip(a, 0, n - 1)
    return ((1 - fx) * (1 - fy) * p[cl(y0, H), cl(x0, W)] + fx * (1 - fy) * p[cl(y0, H), cl(x0 + 1, W)] +
            (1 - fx) * fy * p[cl(y0 + 1, H), cl(x0, W)] + fx * fy * p[cl(y0 + 1, H), cl(x0 + 1, W)])


def test_the_textured_scene_gives_back_its_texture():
    """ortho_scene's block: the mesh of its depth maps (mesh.depth_to_mesh), textured from its rendered images.  A bilinear
    sample of the atlas at a seen face's centroid texcoord is texture(x, y) at the face's centroid within 10 levels (median over
    the faces, the largest channel) and 20 levels for 90 % of them: the mesh lies within about a voxel (0.4 m) of the surface
    and the texture changes by up to 33 levels per metre.  Sampling at other faces' texcoords errs at least 3 times as much.
    Every seen face's texcoords lie inside its chart's rect."""
    from deep3d_aerial_amd import mesh, texture

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    mviews = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda())
              for v in scene.views]
    v, f = mesh.depth_to_mesh(mviews, mesh.MeshGrid(border, voxel))
    ov = _views([dict(s, id=i) for i, s in enumerate(scene.views)])
    res = texture.texture_mesh(v, f, ov, page_size=256)
    key = res["key"].cpu().numpy()
    seen = np.flatnonzero(key != T.EMPTY)
    assert len(seen) > 0.5 * len(key) and len(seen) > 200
    tc, tn = res["texcoord"].cpu().numpy()[seen], res["texnumber"].cpu().numpy()[seen]
    pk = res["packing"]
    P = pk.page_size
    err = np.empty(len(seen))
    Vh, Fh = v.cpu().numpy().astype(np.float64), f.cpu().numpy()[seen]
    g = (Vh[Fh[:, 0]] + Vh[Fh[:, 1]] + Vh[Fh[:, 2]]) / 3
    for k in range(pk.n_pages):
        on = tn == k
        s, t = tc[on][:, 0::2].mean(1), tc[on][:, 1::2].mean(1)
        got = _bilinear(res["pages"][k], s * P - 0.5, (1 - t) * pk.heights[k] - 0.5)
        err[on] = np.abs(got - OS.texture(g[on, 0], g[on, 1])).max(1)
    # the control: each face sampled at another seen face's texcoords
    perm = np.random.default_rng(0).permutation(len(seen))
    ctrl = np.empty(len(seen))
    for k in range(pk.n_pages):
        on = tn[perm] == k
        s, t = tc[perm][on][:, 0::2].mean(1), tc[perm][on][:, 1::2].mean(1)
        got = _bilinear(res["pages"][k], s * P - 0.5, (1 - t) * pk.heights[k] - 0.5)
        ctrl[on] = np.abs(got - OS.texture(g[on, 0], g[on, 1])).max(1)
    print("texture error: median %.2f, 90th percentile %.2f, max %.2f levels; control median %.2f" %
          (np.median(err), np.percentile(err, 90), err.max(), np.median(ctrl)))
    assert np.median(err) <= 10.0 and np.percentile(err, 90) <= 20.0
    assert np.median(ctrl) >= 3 * np.median(err)
    # texcoords inside the rect, in texel units
    chart = res["chart"].cpu().numpy()[seen]
    table = res["table"]
    for k in range(pk.n_pages):
        on = tn == k
        tb = table[chart[on]]
        x = tc[on][:, 0::2] * P - 0.5
        y = (1 - tc[on][:, 1::2]) * pk.heights[k] - 0.5
        assert (x >= tb[:, 4:5] - 1e-3).all() and (x <= (tb[:, 4] + tb[:, 2] - 1)[:, None] + 1e-3).all()
        assert (y >= tb[:, 5:6] - 1e-3).all() and (y <= (tb[:, 5] + tb[:, 3] - 1)[:, None] + 1e-3).all()


def test_inputs_are_checked():
    from deep3d_aerial_amd import texture

    V, F, vs = _random_scene(0, n=8)
    v, f = _mesh(V, F)
    with pytest.raises(ValueError):
        texture.select_faces(v, f + 1000, _views(vs))
    with pytest.raises(RuntimeError):
        texture.select_faces(v.cpu(), f.cpu(), _views(vs))
    with pytest.raises(ValueError):
        texture.texture_mesh(v, f, _views(vs), page_size=100)   # narrower than a view
    with pytest.raises(ValueError):
        texture.select_faces(v, f, _views(vs[:1] + vs[:1]))   # duplicate ids
    key = texture.select_faces(v, f[:0], _views(vs))
    assert key.shape == (0,)
    res = texture.texture_mesh(v, f[:0], _views(vs), page_size=256)
    assert res["packing"].heights == [2] and res["texcoord"].shape == (0, 6)


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "texture_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_textured_mesh_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import texture

    border, voxel = TS.scene_border(OS.ImageSceneViews())
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    _, F, _, tn, files = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    assert len(F) > 100 and files and len(files) == tn.max() + 1
    for name in ["tex.ply", "mesh.ply"] + files:
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name
    # the stage textures the mesh the mesh stage wrote: the same vertices and faces
    from deep3d_aerial_amd import mesh

    Vm, Fm = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    Vt, Ft, _, _, _ = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    assert np.array_equal(Vm, Vt) and np.array_equal(Fm, Ft)


def test_predict_main_fuse_mesh_texture_and_the_standalone_cli(tmp_path):
    """predict --fuse --mesh --texture on the block fixture (seeded casmvsnet weights: plumbing, not geometry) and
    python -m deep3d_aerial_amd.texture on the mesh and the MVS folder predict wrote give the same files."""
    import block_fixture as BF
    from deep3d_aerial_amd import mvs_dl, predict as P, synthetic as S, texture

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    S.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    ply = tmp_path / "mesh" / "block.ply"
    tex = tmp_path / "tex" / "block.ply"
    flags = ["--border=-200,400,-200,200,-600,100", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    tflags = ["--depth_tolerance=0.5", "--page_size=256", "--views_per_batch=2"]
    mvs = tmp_path / "MVS"
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                     "--position_threshold=50", "--mesh", str(ply)] + ["--mesh_" + f[2:] for f in flags] +
                         ["--texture", str(tex)] + ["--texture_" + f[2:] for f in tflags]).run(folder, str(mvs))
    assert tex.exists()
    cli = tmp_path / "cli" / "block.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.texture", "--mesh", str(ply), "--mvs", str(mvs), "--out", str(cli)] +
                         tflags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert cli.read_bytes() == tex.read_bytes()
    _, _, _, _, files = texture.read_textured_ply(str(tex))
    for name in files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "tex" / name).read_bytes()
