"""The kernels of csrc/texture_smooth.hip on the GPU, bit for bit against the numpy restatement of tests/test_texture_smooth.py:
the candidate lists (batching, view order, merge, the selection's key in column 0), the smoothing rounds on a mesh of a rough
grid, a fan, an edge of three faces and a face with a repeated index, texture_mesh(smooth_views=...) against the numpy chain,
and the files written on one and two ranks, by predict and by python -m deep3d_aerial_amd.texture."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_scene as OS
import test_texture as T
import test_texture_smooth as S
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
K = S.K


def _views(vs):
    from deep3d_aerial_amd import ortho

    return [ortho.OrthoView(v["id"], v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["image"]).cuda())
            for v in vs]


def _mesh(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F, np.int32)).cuda()


# ----------------------------------------------------------------------------------------
# candidates
# ----------------------------------------------------------------------------------------
def _candidate_scene():
    """600 faces on z = 10 (three cull blocks of 256, the last partial), jittered, with a flipped and a degenerate face, and 70
    views of 64 x 48 (two mask words, the second partial): 35 crowd over one corner of the mesh, 35 are spread over its near half,
    so the far edge is seen by none; a few depth maps have holes; the last view is the twin of the first under another id."""
    rng = np.random.default_rng(11)
    nx, ny = 20, 15
    ys, xs = np.mgrid[0:ny + 1, 0:nx + 1]
    V = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 10.0)], 1) + rng.uniform(-0.04, 0.04, (xs.size, 3))
    F = []
    for i in range(ny):
        for j in range(nx):
            a, b, c, d = i * (nx + 1) + j, i * (nx + 1) + j + 1, (i + 1) * (nx + 1) + j, (i + 1) * (nx + 1) + j + 1
            F += [[a, c, b], [b, c, d]]   # normals toward -Z, the cameras
    F = np.array(F, np.int32)
    F[5] = F[5][::-1]
    F[9, 2] = F[9, 0]
    vs = []
    for k in range(69):
        C = (rng.uniform(4, 8), rng.uniform(4, 8), rng.uniform(0, 0.5)) if k < 35 else (rng.uniform(0, 9), rng.uniform(0, 9), 0.0)
        v = T.cam_view(int(rng.integers(0, 1 << 30)), C=C, f=float(rng.uniform(30, 50)), depth=10.0)
        if k % 9 == 0:
            v["depth"][rng.uniform(size=v["depth"].shape) < 0.1] = 0.0
        vs.append(v)
    vs.append(dict(vs[0], id=vs[0]["id"] ^ 1))
    assert len({v["id"] for v in vs}) == 70
    return V.astype(np.float32), F, vs


@functools.lru_cache(maxsize=None)
def candidate_scene_value():
    """The candidate scene and the restatement's lists: built once, shared (tests/test_uninitialised_gpu.py uses it too), never
    changed."""
    V, F, vs = _candidate_scene()
    return V, F, vs, S.candidates_numpy(V, F, vs)


@pytest.fixture(scope="module")
def candidate_scene():
    return candidate_scene_value()


def test_the_candidate_scene_covers_full_partial_and_empty_lists(candidate_scene):
    V, F, vs, want = candidate_scene
    passing = np.stack([T.select_numpy(V, F, [v]) != T.EMPTY for v in vs], 1).sum(1)
    assert len(F) == 600 and len(vs) == 70
    assert (passing > K).any() and (passing == 0).any() and ((passing >= 1) & (passing < K)).any()
    assert np.array_equal((want != T.EMPTY).sum(1), np.minimum(passing, K))


@pytest.mark.parametrize("batch,reverse", [(None, False), (1, False), (7, False), (64, False), (70, True), (7, True)])
def test_candidates_are_bit_equal_to_numpy_for_any_batching_and_order(candidate_scene, batch, reverse):
    from deep3d_aerial_amd import texture

    V, F, vs, want = candidate_scene
    v, f = _mesh(V, F)
    got = texture.face_candidates(v, f, _views(vs[::-1] if reverse else vs), views_per_batch=batch).cpu().numpy()
    assert np.array_equal(got, want)
    # rows strictly increasing, then padded
    filled = got != T.EMPTY
    assert (np.diff(filled.astype(np.int8), axis=1) <= 0).all()
    assert (np.diff(got, axis=1)[filled[:, 1:]] > 0).all()


def test_column_0_is_the_selections_key_and_two_halves_merge_to_the_whole(candidate_scene):
    from deep3d_aerial_amd import texture

    V, F, vs, want = candidate_scene
    v, f = _mesh(V, F)
    ov = _views(vs)
    key = texture.select_faces(v, f, ov)
    assert np.array_equal(key.cpu().numpy(), want[:, 0]) and np.array_equal(want[:, 0], T.select_numpy(V, F, vs))
    a, b = texture.face_candidates(v, f, ov[:31]), texture.face_candidates(v, f, ov[31:])
    assert np.array_equal(a.cpu().numpy(), S.candidates_numpy(V, F, vs[:31]))
    merged = texture.merge_candidates(a, b)
    assert merged is a and np.array_equal(merged.cpu().numpy(), want)
    # a view handed over twice counts once
    again = texture.face_candidates(v, f, ov[:5], cand=merged.clone())
    assert np.array_equal(again.cpu().numpy(), want)
    assert np.array_equal(texture.merge_candidates(again, merged).cpu().numpy(), want)


# ----------------------------------------------------------------------------------------
# smoothing
# ----------------------------------------------------------------------------------------
def _smooth_scene():
    """The N = 12 rough grid (288 faces with its own candidates, some rows cut short, some emptied), then a fan of 40 faces round
    one vertex, three faces on one edge and a face with a repeated index, their rows 1 .. 16 random keys with s in [1, 2)."""
    rng = np.random.default_rng(5)
    Vg, Fg, cg = S.rough_grid(12)
    cg = cg.copy()
    for f in rng.choice(len(Fg), 60, replace=False):
        cg[f, rng.integers(1, K):] = T.EMPTY
    cg[rng.choice(len(Fg), 10, replace=False)] = T.EMPTY
    n0 = len(Vg)
    hub, rim = n0, n0 + 1 + np.arange(40)
    fan = np.stack([np.full(40, hub), rim, np.roll(rim, -1)], 1)
    e0, e1 = n0 + 41, n0 + 42
    book = np.array([[e0, e1, n0 + 43], [e0, e1, n0 + 44], [e1, e0, n0 + 45]])
    bad = np.array([[n0 + 43, n0 + 43, n0 + 44]])
    extra = np.concatenate([fan, book, bad]).astype(np.int32)
    ce = np.full((len(extra), K), T.EMPTY, np.int64)
    for f in range(len(extra)):
        L = 1 + (f % K)
        s = np.sort(rng.uniform(1.0, 2.0, L).astype(np.float32))
        ce[f, :L] = np.sort(T.make_key(s, rng.permutation(6 if L <= 6 else K)[:L]))
    ce[7] = T.EMPTY
    F = np.concatenate([Fg, extra]).astype(np.int32)
    cand = np.ascontiguousarray(np.concatenate([cg, ce]))
    assert (np.diff(cand, axis=1)[cand[:, 1:] != T.EMPTY] > 0).all()
    return F, n0 + 46, cand


@functools.lru_cache(maxsize=None)
def smooth_scene_value():
    """The smoothing scene and the restatement's state after every round: built once, shared, never changed."""
    F, n, cand = _smooth_scene()
    states = list(S.smooth_rounds_numpy(F, cand, 0.1, 0.25, 64))
    return F, n, cand, states


@pytest.fixture(scope="module")
def smooth_scene():
    return smooth_scene_value()


def test_the_smooth_scene_runs_past_one_host_read_and_holds_every_row_kind(smooth_scene):
    F, n, cand, states = smooth_scene
    assert len(F) == 288 + 44 and len(F) > 256   # two workgroups
    assert not states[-1][1].any() and len(states) - 1 > 9, len(states)
    assert set((cand != T.EMPTY).sum(1).tolist()) == set(range(K + 1))
    label = states[-1][0]
    assert (label > 0).sum() > 50 and (label[288:] > 0).any() and label[-1] == -1


@pytest.mark.parametrize("rounds", [1, 2, 3, 9, 64])
def test_smoothing_is_bit_equal_to_numpy_after_any_number_of_rounds(smooth_scene, rounds):
    from deep3d_aerial_amd import texture

    F, n, cand, states = smooth_scene
    f, c = torch.from_numpy(F).cuda(), torch.from_numpy(cand).cuda()
    key, label, commits = texture.smooth_views(f, n, c, 0.1, 0.25, rounds)
    want_key, want_label, want_commits = S.smooth_numpy(F, cand, 0.1, 0.25, rounds)
    assert np.array_equal(label.cpu().numpy(), want_label)
    assert np.array_equal(key.cpu().numpy(), want_key)
    assert np.array_equal(commits.cpu().numpy(), want_commits)
    if rounds < len(states) - 1:   # capped below the fixed point: the state after `rounds` rounds, not the final one
        assert len(want_commits) == rounds and np.array_equal(want_label, states[rounds - 1][0])
        assert not np.array_equal(want_label, states[-1][0])
    else:
        assert np.array_equal(want_label, states[-1][0]) and len(commits) == len(states) - 1
    assert torch.equal(c, torch.from_numpy(cand).cuda())   # the candidates are read only


def test_other_settings_and_a_second_run_give_the_same_bits(smooth_scene):
    from deep3d_aerial_amd import texture

    F, n, cand, _ = smooth_scene
    f, c = torch.from_numpy(F).cuda(), torch.from_numpy(cand).cuda()
    for weight, max_loss in ((0.1, 1.0), (0.03, 0.1), (1e-30, 0.25)):
        got = texture.smooth_views(f, n, c, weight, max_loss, 128)
        again = texture.smooth_views(f, n, c, weight, max_loss, 128)
        want = S.smooth_numpy(F, cand, weight, max_loss, 128)
        for g, a, w in zip(got, again, want):
            assert np.array_equal(g.cpu().numpy(), w) and torch.equal(g, a)
    assert len(want[2]) == 0 and (want[1] <= 0).all()   # a vanishing weight leaves every label at 0
    with pytest.raises(ValueError):
        texture.smooth_views(f, n, c[:-1].contiguous(), 0.1)
    with pytest.raises(ValueError):
        texture.smooth_views(f, n - 40, c, 0.1)   # an index past the vertices
    key, label, commits = texture.smooth_views(f[:0], n, c[:0], 0.1)
    assert key.shape == (0,) and label.shape == (0,) and commits.shape == (0,)


# ----------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------
def test_texture_mesh_with_smoothing_equals_the_numpy_chain_on_the_block():
    from deep3d_aerial_amd import mesh, texture

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    mviews = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda())
              for v in scene.views]
    v, f = mesh.depth_to_mesh(mviews, mesh.MeshGrid(border, voxel))
    vs = [dict(s, id=i) for i, s in enumerate(scene.views)]
    ov = _views(vs)
    got = texture.texture_mesh(v, f, ov, page_size=256, smooth_views={"weight": 0.1})
    plain = texture.texture_mesh(v, f, ov, page_size=256)
    V, F = v.cpu().numpy(), f.cpu().numpy()
    cand = S.candidates_numpy(V, F, vs)
    key, label, commits = S.smooth_numpy(F, cand, 0.1, 0.25, 64)
    assert np.array_equal(got["cand"].cpu().numpy(), cand) and np.array_equal(got["label"].cpu().numpy(), label)
    assert np.array_equal(got["key"].cpu().numpy(), key)
    chart, labels = T.charts_numpy(F, key)
    rects = T.rects_numpy(V, F, key, chart, len(labels), vs, 2)
    packing = texture.pack(rects, 256)
    pages = T.atlas_numpy(rects, packing, (key[labels] & 0xffffffff).astype(np.int64), vs)
    tc, tn = T.texcoords_numpy(V, F, key, chart, rects, packing, vs)
    assert np.array_equal(got["chart"].cpu().numpy(), chart) and np.array_equal(got["labels"].cpu().numpy(), labels)
    assert np.array_equal(got["rects"].cpu().numpy(), rects)
    assert np.array_equal(got["packing"].place, packing.place) and got["packing"].heights == packing.heights
    assert len(got["pages"]) == len(pages) and all(np.array_equal(a, b) for a, b in zip(got["pages"], pages))
    assert np.array_equal(got["texcoord"].cpu().numpy().view(np.uint32), tc.view(np.uint32))
    assert np.array_equal(got["texnumber"].cpu().numpy(), tn)
    # every face's key is one of its candidates; faces without a winner keep none
    none = cand[:, 0] == T.EMPTY
    assert (key[none] == T.EMPTY).all() and (label[none] == -1).all() and none.any()
    assert (cand[~none] == key[~none, None]).any(1).all()
    # no more charts than the unsmoothed run, which is what "smooth" reports; the unsmoothed run itself is unchanged
    info = got["smooth"]
    n_plain = int(plain["labels"].shape[0])
    print("block: %d faces, %d charts -> %d in %d rounds, mean loss %.4f, largest %.4f" %
          (len(F), n_plain, len(labels), info["rounds"], info["mean_loss"], info["max_loss"]))
    assert np.array_equal(plain["key"].cpu().numpy(), cand[:, 0]) and "smooth" not in plain and "label" not in plain
    assert info["charts_before"] == n_plain and len(labels) <= n_plain
    assert info["rounds"] == len(commits) and info["converged"] and info["commits"] == commits.tolist()
    assert 0 <= info["mean_loss"] <= info["max_loss"] <= 0.25


def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "texture_smooth_scene.py"), str(out_dir),
           ",".join(repr(b) for b in border), repr(voxel)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_smoothed_texture_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import texture

    border, voxel = TS.scene_border(OS.ImageSceneViews())
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    _, F, _, tn, files = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    assert len(F) > 100 and files and len(files) == tn.max() + 1
    for name in ["tex.ply", "mesh.ply"] + files:
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name


def test_predict_and_the_standalone_cli_write_the_smoothed_texture(tmp_path):
    """predict --fuse --mesh --texture --texture_smooth_views 0.1 on the block fixture (seeded casmvsnet weights: plumbing, not
    geometry) and python -m deep3d_aerial_amd.texture --smooth_views 0.1 on the mesh and the MVS folder predict wrote: both
    write a PLY that read_textured_ply reads back, and the same one."""
    import block_fixture as BF
    from deep3d_aerial_amd import mvs_dl, predict as P, synthetic as Sy, texture

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    Sy.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    ply = tmp_path / "mesh" / "block.ply"
    tex = tmp_path / "tex" / "block.ply"
    flags = ["--border=-200,400,-200,200,-600,100", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    tflags = ["--depth_tolerance=0.5", "--page_size=256", "--views_per_batch=2", "--smooth_views=0.1", "--smooth_rounds=32"]
    mvs = tmp_path / "MVS"
    mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                         extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                     "--position_threshold=50", "--mesh", str(ply)] + ["--mesh_" + f[2:] for f in flags] +
                         ["--texture", str(tex)] + ["--texture_" + f[2:] for f in tflags]).run(folder, str(mvs))
    Vt, Ft, tc, tn, files = texture.read_textured_ply(str(tex))
    assert files and tc.shape == (len(Ft), 6) and tn.shape == (len(Ft),)
    cli = tmp_path / "cli" / "block.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.texture", "--mesh", str(ply), "--mvs", str(mvs), "--out", str(cli)] +
                         tflags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "smoothed the view choice" in res.stdout
    assert len(texture.read_textured_ply(str(cli))[1]) == len(Ft)
    assert cli.read_bytes() == tex.read_bytes()
    for name in files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "tex" / name).read_bytes()
