"""The kernels of csrc/texture_outliers.hip on the GPU, bit for bit against the numpy restatement of tests/test_texture_outliers.py:
the colour words (batching, view order, accumulation, absent views), the vote on crafted rows (every list length, ties, slots
without a colour, in place), the behaviour on a scene whose honest images agree and whose painted view does not,
texture_mesh(outliers=...) against the numpy chain with and without the smoothing, and the files written on one and two ranks, by
predict and by python -m deep3d_aerial_amd.texture."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_texture as T
import test_texture_outliers as O
import test_texture_smooth as S
import test_texture_smooth_gpu as G
import texture_outliers_scene as XS
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
K = S.K
_views, _mesh = G._views, G._mesh


# ----------------------------------------------------------------------------------------
# colours
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def color_scene():
    V, F, vs = G._candidate_scene()
    cand = S.candidates_numpy(V, F, vs)
    return V, F, vs, cand, O.colors_numpy(V, F, cand, vs)


def test_the_colour_scene_has_a_partial_last_workgroup_and_every_list_kind(color_scene):
    V, F, vs, cand, want = color_scene
    assert len(F) == 600 and len(F) % 256 != 0 and (len(F) * K) % 256 != 0 and len(vs) == 70
    filled = (cand != T.EMPTY).sum(1)
    assert (filled == K).any() and (filled == 0).any() and ((filled > 0) & (filled < K)).any()
    assert np.array_equal(want != 0, cand != T.EMPTY)   # every candidate view shows its face
    assert len(np.unique(want[want != 0])) > 1000


@pytest.mark.parametrize("batch,reverse", [(None, False), (1, False), (7, False), (70, False), (70, True), (7, True)])
def test_colours_are_bit_equal_to_numpy_for_any_batching_and_order(color_scene, batch, reverse):
    from deep3d_aerial_amd import texture

    V, F, vs, cand, want = color_scene
    v, f = _mesh(V, F)
    c = torch.from_numpy(cand).cuda()
    got = texture.face_colors(v, f, c, _views(vs[::-1] if reverse else vs), views_per_batch=batch)
    assert got.dtype == torch.int32 and tuple(got.shape) == (600, K)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(c, torch.from_numpy(cand).cuda())   # the candidates are read only


def test_two_halves_accumulate_to_the_whole_and_absent_views_leave_their_slots(color_scene):
    from deep3d_aerial_amd import texture

    V, F, vs, cand, want = color_scene
    v, f = _mesh(V, F)
    c = torch.from_numpy(cand).cuda()
    ov = _views(vs)
    half = texture.face_colors(v, f, c, ov[:31])
    assert np.array_equal(half.cpu().numpy(), O.colors_numpy(V, F, cand, vs[:31]))
    both = texture.face_colors(v, f, c, ov[31:], col=half)
    assert both is half and np.array_equal(both.cpu().numpy(), want)
    # ten views left out: exactly their slots stay 0
    out_ids = np.array([x["id"] for x in vs[5:65:6]])
    assert len(out_ids) == 10
    rest = [o for o in ov if o.id not in set(out_ids.tolist())]
    got = texture.face_colors(v, f, c, rest).cpu().numpy()
    absent = (cand != T.EMPTY) & np.isin(cand & 0xffffffff, out_ids)
    assert absent.any() and (got[absent] == 0).all() and np.array_equal(got[~absent], want[~absent])
    # a slot that holds something is left as it was when its view is not offered
    marked = torch.full((600, K), 7, dtype=torch.int32, device="cuda")
    got = texture.face_colors(v, f, c, rest, col=marked).cpu().numpy()
    keys = cand != T.EMPTY
    assert (got[absent] == 7).all() and (got[~keys] == 7).all() and np.array_equal(got[keys & ~absent], want[keys & ~absent])
    # no views, no faces
    assert not texture.face_colors(v, f, c, []).any()
    assert tuple(texture.face_colors(v, f[:0], c[:0], ov[:3]).shape) == (0, K)
    with pytest.raises(ValueError):
        texture.face_colors(v, f, c[:-1].contiguous(), ov[:3])


# ----------------------------------------------------------------------------------------
# the vote
# ----------------------------------------------------------------------------------------
def _crafted_rows():
    """4089 rows of random length 0 .. 16 whose channels come from a few clusters plus noise (ties and equal values in every
    channel), some slots without a colour, and the hand-built rows of tests/test_texture_outliers.py: 4099 faces, so the last
    wave is partial."""
    rng = np.random.default_rng(17)
    m = 4089
    cand = np.full((m, K), T.EMPTY, np.int64)
    col = np.zeros((m, K), np.int32)
    centres = np.array([[400, 400, 400], [400, 460, 400], [470, 400, 340], [900, 100, 500], [0, 0, 0], [1020, 1020, 1020]])
    for f in range(m):
        L = f % (K + 1) if f < 200 else int(rng.integers(0, K + 1))
        s = np.sort(rng.uniform(1.0, 2.0, L).astype(np.float32))
        cand[f, :L] = np.sort(T.make_key(s, rng.permutation(40)[:L]))
        kind = rng.integers(0, 4)
        q = centres[rng.integers(0, 2 if kind == 0 else len(centres), L)]
        if kind >= 2:
            q = q + rng.integers(-70, 71, (L, 3))
        if kind == 3:
            q = rng.integers(0, 1021, (L, 3))
        col[f, :L] = O.color_word(np.clip(q, 0, 1020))
        col[f, :L][rng.uniform(size=L) < 0.1] = 0
    hc, hw = O.hand_built_rows()
    cand, col = np.concatenate([cand, hc]), np.concatenate([col, hw])
    assert (np.diff(cand, axis=1)[cand[:, 1:] != T.EMPTY] > 0).all()
    return np.ascontiguousarray(cand), np.ascontiguousarray(col)


@functools.lru_cache(maxsize=None)
def crafted_rows_value():
    """The crafted rows and the restatement's vote at the three thresholds: built once, shared, never changed."""
    cand, col = _crafted_rows()
    return cand, col, {t: O.reject_numpy(cand, col, t) for t in (0.001, 0.06, 1.0)}


@pytest.fixture(scope="module")
def crafted_rows():
    return crafted_rows_value()


def test_the_crafted_rows_hold_every_case(crafted_rows):
    cand, col, want = crafted_rows
    assert len(cand) == 4099 and len(cand) % 64 != 0
    valid, n, dev = O.deviations(cand, col)
    assert set(n.tolist()) == set(range(K + 1))
    assert ((cand != T.EMPTY) & (col == 0)).any()
    q = O.channels(col)
    ties = [sum(len(set(q[f, valid[f], c].tolist())) < n[f] for f in range(len(cand))) for c in range(3)]
    assert all(t > 500 for t in ties)
    for t, (out, rej, counts) in want.items():
        print("threshold %g: tested %d, changed %d, removed %d, kept_all %d" % ((t,) + tuple(counts)))
    assert want[0.06][2][1] > 100 and want[0.06][2][2] > 1000 and want[0.06][2][3] > 10
    # (a tighter threshold does not remove more: more faces lose every view and so keep them all)
    assert want[0.001][2][2] > 1000 and want[0.001][2][3] > want[0.06][2][3] and want[1.0][2][2] == 0 and np.array_equal(want[1.0][0], cand)


@pytest.mark.parametrize("threshold", [0.001, 0.06, 1.0])
def test_the_vote_is_bit_equal_to_numpy_in_place_and_out_of_place(crafted_rows, threshold):
    from deep3d_aerial_amd import texture

    cand, col, want = crafted_rows
    want_out, want_rej, want_counts = want[threshold]
    c, w = torch.from_numpy(cand).cuda(), torch.from_numpy(col).cuda()
    out, rej, counts = texture.reject_outliers(c, w, threshold)
    assert out.data_ptr() != c.data_ptr() and torch.equal(c, torch.from_numpy(cand).cuda())
    assert np.array_equal(out.cpu().numpy(), want_out)
    assert np.array_equal(rej.cpu().numpy(), want_rej)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    same, rej2, counts2 = texture.reject_outliers(c, w, threshold, out=c)
    assert same is c and torch.equal(c, out) and torch.equal(rej2, rej) and torch.equal(counts2, counts)
    assert torch.equal(w, torch.from_numpy(col).cuda())   # the colours are read only


def test_the_vote_of_no_faces_and_bad_arguments():
    from deep3d_aerial_amd import texture

    c, w = torch.zeros((0, K), dtype=torch.int64, device="cuda"), torch.zeros((0, K), dtype=torch.int32, device="cuda")
    out, rej, counts = texture.reject_outliers(c, w, 0.06)
    assert tuple(out.shape) == (0, K) and tuple(rej.shape) == (0,) and counts.tolist() == [0, 0, 0, 0]
    c, w = torch.zeros((3, K), dtype=torch.int64, device="cuda"), torch.zeros((3, K), dtype=torch.int32, device="cuda")
    for bad in (0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            texture.reject_outliers(c, w, bad)
    with pytest.raises(ValueError):
        texture.reject_outliers(c, w[:2].contiguous(), 0.06)
    with pytest.raises(ValueError):
        texture.reject_outliers(c, w.long(), 0.06)


# ----------------------------------------------------------------------------------------
# behaviour
# ----------------------------------------------------------------------------------------
def test_honest_views_lose_nothing_and_a_painted_view_loses_the_faces_it_spoils():
    from deep3d_aerial_amd import texture

    V, F, vs = O.behaviour_scene()
    v, f = _mesh(V, F)
    cand = S.candidates_numpy(V, F, vs)
    res = texture.texture_mesh(v, f, _views(vs), page_size=256, outliers={"threshold": 0.06})
    col = O.colors_numpy(V, F, cand, vs)
    want_out, want_rej, want_counts = O.reject_numpy(cand, col, 0.06)
    assert not want_rej.any() and np.array_equal(want_out, cand)
    assert np.array_equal(res["cand"].cpu().numpy(), cand) and not res["rejected"].any()
    assert np.array_equal(res["key"].cpu().numpy(), texture.select_faces(v, f, _views(vs)).cpu().numpy())
    assert res["outliers"] == {"threshold": 0.06, "T": 61, "faces": 600, "tested": 600, "changed": 0, "removed": 0, "kept_all": 0}
    # the view that wins most faces now lies about the middle of its image
    win = O.winning_view(cand)
    painted = [O.paint(x) if x["id"] == win else x for x in vs]
    c = torch.from_numpy(cand).cuda()
    col2 = texture.face_colors(v, f, c, _views(painted))
    want_col2 = O.colors_numpy(V, F, cand, painted)
    assert np.array_equal(col2.cpu().numpy(), want_col2)
    out, rej, counts = texture.reject_outliers(c, col2, 0.06)
    want_out, want_rej, want_counts = O.reject_numpy(cand, want_col2, 0.06)
    out, rej = out.cpu().numpy(), rej.cpu().numpy()
    assert np.array_equal(out, want_out) and np.array_equal(rej, want_rej) and np.array_equal(counts.cpu().numpy(), want_counts)
    bits = ((rej[:, None] >> np.arange(K)) & 1).astype(bool)
    assert not (bits & (want_col2 == col)).any()   # no slot whose colour did not change is removed
    first = bits[:, 0]
    assert np.array_equal(out[first, 0], cand[first, 1])   # a face that lost its first view now holds its old second key
    touched = (want_col2 != col).any(1)
    print("painted view %d: %d faces touched, %d lose it" % (win, touched.sum(), (rej != 0).sum()))
    assert (rej != 0).sum() > 100


# ----------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block():
    """The painted block's mesh, its views, and the restatement's filtered candidate lists."""
    from deep3d_aerial_amd import mesh

    scene = XS.painted_scene()
    border, voxel = TS.scene_border(scene)
    mviews = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda())
              for v in scene.views]
    v, f = mesh.depth_to_mesh(mviews, mesh.MeshGrid(border, voxel))
    vs = [dict(s, id=i) for i, s in enumerate(scene.views)]
    V, F = v.cpu().numpy(), f.cpu().numpy()
    cand = S.candidates_numpy(V, F, vs)
    col = O.colors_numpy(V, F, cand, vs)
    return v, f, vs, cand, col, O.reject_numpy(cand, col, 0.06)


@pytest.mark.parametrize("smooth", [False, True])
def test_texture_mesh_with_outliers_equals_the_numpy_chain_on_the_block(block, smooth):
    from deep3d_aerial_amd import texture

    v, f, vs, cand, col, (cand_out, rejected, counts) = block
    V, F = v.cpu().numpy(), f.cpu().numpy()
    ov = _views(vs)
    got = texture.texture_mesh(v, f, ov, page_size=256, outliers={"threshold": 0.06}, smooth_views={"weight": 0.1} if smooth else None)
    assert np.array_equal(got["cand"].cpu().numpy(), cand_out) and np.array_equal(got["rejected"].cpu().numpy(), rejected)
    info = got["outliers"]
    print("block: %d faces, %s" % (len(F), info))
    assert [info["tested"], info["changed"], info["removed"], info["kept_all"]] == counts.tolist() and info["faces"] == len(F)
    assert info["removed"] > 0 and info["changed"] > 0   # the painted view makes the filter act
    if smooth:
        key, label, commits = S.smooth_numpy(F, cand_out, 0.1, 0.25, 64)
        assert np.array_equal(got["label"].cpu().numpy(), label) and got["smooth"]["commits"] == commits.tolist()
        assert got["smooth"]["charts_before"] == len(T.charts_numpy(F, cand_out[:, 0])[1])
    else:
        key = cand_out[:, 0]
        assert "label" not in got and "smooth" not in got
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
    if not smooth:   # with the filter off the run is what it was: the selection's key, no new entries
        plain = texture.texture_mesh(v, f, ov, page_size=256)
        assert np.array_equal(plain["key"].cpu().numpy(), cand[:, 0]) and not {"cand", "rejected", "outliers"} & set(plain)
        assert not np.array_equal(plain["key"].cpu().numpy(), key)


def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "texture_outliers_scene.py"), str(out_dir),
           ",".join(repr(b) for b in border), repr(voxel)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_filtered_texture_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import texture

    border, voxel = TS.scene_border(XS.painted_scene())
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    _, F, _, tn, files = texture.read_textured_ply(str(tmp_path / "one" / "tex.ply"))
    assert len(F) > 100 and files and len(files) == tn.max() + 1
    for name in ["tex.ply", "mesh.ply"] + files:
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "two" / name).read_bytes(), name


def test_predict_and_the_standalone_cli_write_the_filtered_texture(tmp_path):
    """predict --fuse --mesh --texture --texture_outlier_threshold 0.06 on the block fixture (seeded casmvsnet weights: plumbing,
    not geometry) and python -m deep3d_aerial_amd.texture --outlier_threshold 0.06 on the mesh and the MVS folder predict wrote:
    both write a PLY that read_textured_ply reads back, and the same one."""
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
    tflags = ["--depth_tolerance=0.5", "--page_size=256", "--views_per_batch=2", "--outlier_threshold=0.06"]
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
    assert "rejected outlier views" in res.stdout
    assert len(texture.read_textured_ply(str(cli))[1]) == len(Ft)
    assert cli.read_bytes() == tex.read_bytes()
    for name in files:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "tex" / name).read_bytes()
