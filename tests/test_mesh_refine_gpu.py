"""The kernels of csrc/mesh_refine.hip on the GPU, bit for bit against the numpy restatement of tests/test_mesh_refine.py on the
scene of tests/mesh_refine_scene.py: frames, view lists (batching, order, halves), the pick, the relaxed displacement and the moved
vertices for reach 1, 4 and 7; absent views; refine_mesh over two scales and its effect; and the files written by predict, by
python -m deep3d_aerial_amd.refine and on one and two ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_refine_scene as RS
import test_mesh_refine as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EMPTY = R.EMPTY
_CHAINS = {}


def _views(vs):
    from deep3d_aerial_amd import ortho

    return [ortho.OrthoView(v["id"], v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["image"]).cuda())
            for v in vs]


def _mesh(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F, np.int32)).cuda()


def chain(reach):
    """One scale of the restatement on the scene with this reach (reach 4: the first scale of the shared chain)."""
    s = R.scene()
    if reach not in _CHAINS:
        if reach == RS.REACH:
            _CHAINS[reach] = s["detail"][0]
        else:
            detail = []
            R.refine_numpy(s["V0"], s["F"], s["views"], RS.STEP, RS.SPACING, reach=reach, scales=1, detail=detail)
            _CHAINS[reach] = detail[0]
    return s, _CHAINS[reach]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    return np.array_equal(_bits(got.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("reach", [1, 4, 7])
@pytest.mark.parametrize("batch,reverse", [(None, False), (2, False), (None, True)])
def test_every_pass_is_bit_equal_to_numpy(reach, batch, reverse):
    from deep3d_aerial_amd import refine

    s, want = chain(reach)
    v, f = _mesh(s["V0"], s["F"])
    ov = _views(s["views"][::-1] if reverse else s["views"])
    topo = refine.Topology(f, int(v.shape[0]))
    frame, active = refine.vertex_frames(v, f, topo)
    assert _same(frame, want["frame"]) and _same(active, want["active"])
    lists = refine.vertex_views(v, frame, active, ov, RS.STEP, reach, views_per_batch=batch)
    assert _same(lists, want["lists"])
    kstar, weight, d0, counts = refine.match(v, frame, active, lists, ov, RS.STEP, RS.SPACING, reach)
    assert _same(kstar, want["kstar"]) and _same(weight, want["weight"]) and _same(d0, want["d0"])
    assert counts.cpu().tolist() == want["counts"].tolist()
    d = refine.relax(weight, d0, active, topo)
    assert _same(d, want["d"])
    out = refine.apply(v, frame, active, d)
    assert _same(out, want["out"])
    assert _same(v, s["V0"]) and _same(f, s["F"])   # the inputs are read only
    inactive = want["active"] == 0
    assert inactive.any() and np.array_equal(out.cpu().numpy()[inactive].view(np.uint32), s["V0"][inactive].view(np.uint32))
    if reach == 1:
        assert ((want["kstar"] == 0) | (want["kstar"] == 2)).sum() > 100   # three hypotheses for a displacement of three steps: ends


def test_two_halves_of_the_views_merge_to_the_whole_list():
    from deep3d_aerial_amd import refine

    s, want = chain(RS.REACH)
    v, f = _mesh(s["V0"], s["F"])
    ov = _views(s["views"])
    frame, active = torch.from_numpy(want["frame"]).cuda(), torch.from_numpy(want["active"]).cuda()
    half = refine.vertex_views(v, frame, active, ov[4:], RS.STEP)
    assert _same(half, R.views_numpy(s["V0"], want["frame"], want["active"], s["views"][4:], RS.STEP)) and not _same(half, want["lists"])
    both = refine.vertex_views(v, frame, active, ov[:4], RS.STEP, lists=half)
    assert both is half and _same(both, want["lists"])
    again = refine.vertex_views(v, frame, active, ov, RS.STEP, lists=both.clone())   # keys the list holds are counted once
    assert _same(again, want["lists"])
    assert _same(refine.vertex_views(v, frame, active, [], RS.STEP), np.full_like(want["lists"], EMPTY))


def test_views_absent_from_the_table_leave_the_vertices_that_do_not_list_them():
    from deep3d_aerial_amd import refine

    s, want = chain(RS.REACH)
    v, _ = _mesh(s["V0"], s["F"])
    frame, active = torch.from_numpy(want["frame"]).cuda(), torch.from_numpy(want["active"]).cuda()
    lists = torch.from_numpy(want["lists"]).cuda()
    gone = {2, 5}
    rest = [x for x in s["views"] if x["id"] not in gone]
    k, w, d0, counts = refine.match(v, frame, active, lists, _views(rest), RS.STEP, RS.SPACING, RS.REACH)
    wk, ww, wd0, wcounts = R.match_numpy(s["V0"], want["frame"], want["active"], want["lists"], rest, RS.STEP, RS.SPACING, RS.REACH)
    assert _same(k, wk) and _same(w, ww) and _same(d0, wd0) and counts.cpu().tolist() == wcounts.tolist()
    listed = ((want["lists"] != EMPTY) & np.isin(want["lists"] & 0xffffffff, list(gone))).any(1)
    assert listed.any() and (~listed & (want["kstar"] >= 0)).any()
    assert np.array_equal(wk[~listed], want["kstar"][~listed]) and np.array_equal(wd0[~listed].view(np.uint32), want["d0"][~listed].view(np.uint32))
    assert not np.array_equal(wk[listed], want["kstar"][listed])
    # a view without an image is absent too; no view at all: nothing matches
    k0, w0, _, c0 = refine.match(v, frame, active, lists, [], RS.STEP, RS.SPACING, RS.REACH)
    assert (k0 == -1).all() and not w0.any() and c0.cpu().tolist() == [int(wcounts[0]), int(wcounts[1]), 0, 0]


def test_refine_mesh_over_two_scales_equals_the_chain_and_halves_the_distance():
    from deep3d_aerial_amd import refine

    s = R.scene()
    v, f = _mesh(s["V0"], s["F"])
    f0 = f.clone()
    out, info = refine.refine_mesh(v, f, _views(s["views"]), views_per_batch=3, **RS.SETTINGS)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(v.shape) and torch.equal(f, f0) and _same(v, s["V0"])
    assert _same(out, s["out"])
    assert len(info["scales"]) == 2 and info["vertices"] == len(s["V0"])
    for got, want in zip(info["scales"], s["detail"]):
        assert [got["active"], got["two_views"], got["matched"], got["moved"]] == want["counts"].tolist()
        assert got["step"] == want["step"] and got["spacing"] == want["spacing"]
    active = s["detail"][0]["active"] != 0
    before, after = R.rms_ratio(s["V0"], out.cpu().numpy(), active)
    print("GPU: rms distance to the plane %.4f -> %.4f (ratio %.4f)" % (before, after, after / before))
    assert after <= 0.5 * before
    assert np.array_equal(out.cpu().numpy()[~active].view(np.uint32), s["V0"][~active].view(np.uint32))
    one, _ = refine.refine_mesh(v, f, _views(s["views"]), scales=1, **RS.SETTINGS)
    assert _same(one, s["detail"][0]["out"])


def test_no_vertices_and_bad_arguments_launch_nothing():
    import ctypes

    from deep3d_aerial_amd import _lib, refine

    lib = _lib.load()
    t = torch.zeros((64,), dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.d3d_mesh_refine_frames(p, 0, p, 0, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3d_mesh_refine_match(p, 0, p, p, p, p, 0, 4, 0.5, 0.5, 360000, 0.6, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3d_mesh_refine_match(p, 4, p, p, p, p, 0, 8, 0.5, 0.5, 360000, 0.6, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3d_mesh_refine_relax(p, p, p, p, p, 0, 1.0, 10, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.d3d_mesh_refine_apply(p, 0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not t.any()
    v, f = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    out, info = refine.refine_mesh(v, f, [], 0.5)
    assert out is v and info == {"scales": [], "vertices": 0}
    s = R.scene()
    v, f = _mesh(s["V0"], s["F"])
    for bad in ({"reach": 0}, {"reach": 8}, {"scales": 0}, {"scales": 9}, {"spacing": float("nan")}):
        with pytest.raises(ValueError):
            refine.refine_mesh(v, f, [], 0.5, **bad)
    with pytest.raises(ValueError):
        refine.refine_mesh(v, f, [], 0.0)
    with pytest.raises(ValueError):
        refine.vertex_views(v, torch.zeros((3, 9), dtype=torch.float64, device="cuda"), torch.zeros((len(v),), dtype=torch.uint8, device="cuda"),
                            [], 0.5)


# ----------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def _launch(n_ranks, out_dir, border, voxel, step):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mesh_refine_scene.py"), str(out_dir),
           ",".join(repr(b) for b in border), repr(voxel), repr(step)]
    res = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_refined_mesh_one_rank_writes(tmp_path):
    from deep3d_aerial_amd import mesh, refine

    scene = RS.RefineSceneViews()
    border, voxel = RS.mesh_border(scene)
    out1 = _launch(1, tmp_path / "one", border, voxel, voxel / 2)
    out2 = _launch(2, tmp_path / "two", border, voxel, voxel / 2)
    assert "rank 0/1 mesh_refine" in out1 and "rank 0/2 mesh_refine" in out2 and "rank 1/2" in out2
    one = (tmp_path / "one" / "mesh.ply").read_bytes()
    assert one == (tmp_path / "two" / "mesh.ply").read_bytes()
    # it is the mesh stage's mesh, refined: the same faces, the vertices refine_mesh gives
    mviews = [mesh.MeshView(v["K"], v["E"], torch.from_numpy(v["depth"]).cuda(), torch.from_numpy(v["confidence"]).cuda())
              for v in scene.views]
    v, f = mesh.depth_to_mesh(mviews, mesh.MeshGrid(border, voxel))
    V, F = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    assert len(F) > 100 and np.array_equal(F, f.cpu().numpy()) and not np.array_equal(V, v.cpu().numpy())
    want, info = refine.refine_mesh(v, f, _views(RS.numpy_views(scene)), voxel / 2)
    assert info["scales"][0]["moved"] > 0 and _same(want, V)


def test_predict_and_the_standalone_cli_write_the_same_refined_mesh(tmp_path):
    """predict --fuse --mesh on the block fixture (seeded casmvsnet weights: plumbing, not geometry) without and with --mesh_refine,
    and python -m deep3d_aerial_amd.refine on the unrefined mesh and the MVS folder predict wrote: without the flag the PLY is the
    mesh stage's own, with it predict and the command line write the same bytes."""
    import block_fixture as BF
    from deep3d_aerial_amd import mesh, mvs_dl, predict as P, synthetic as Sy

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    Sy.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    # the fixture's cameras look along +z at ground 500 m away: this border holds it (the seeded weights' depths lie in 430 .. 590)
    flags = ["--border=-200,400,-200,200,400,600", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    rflags = ["--reach=3", "--spacing=4", "--min_score=-1", "--smooth_iterations=4"]
    plys = {}
    for name, extra in (("plain", []), ("refined", ["--mesh_refine", "5"] + ["--mesh_refine_" + r[2:] for r in rflags])):
        plys[name] = tmp_path / name / "block.ply"
        mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                             extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                         "--position_threshold=50", "--mesh", str(plys[name])] + ["--mesh_" + f[2:] for f in flags] +
                             extra).run(folder, str(tmp_path / name / "MVS"))
    direct = tmp_path / "direct" / "block.ply"
    import argparse

    ap = argparse.ArgumentParser()
    mesh.add_arguments(ap)
    a = ap.parse_args(flags)
    mesh.build_and_write(mesh.load_mvs_views(str(tmp_path / "plain" / "MVS")), mesh.settings_from_args(a, str(direct)))
    assert direct.read_bytes() == plys["plain"].read_bytes()
    cli = tmp_path / "cli" / "block.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.refine", "--mesh", str(plys["plain"]), "--mvs", str(tmp_path / "plain" / "MVS"),
                          "--out", str(cli), "--step", "5"] + rflags, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "refined mesh" in res.stdout
    V0, F0 = mesh.read_ply(str(plys["plain"]))
    V1, F1 = mesh.read_ply(str(plys["refined"]))
    moved = int((V0 != V1).any(1).sum())
    print("block: %d vertices, %d faces, %d vertices moved by the refinement" % (len(V0), len(F0), moved))
    assert len(V0) > 100 and len(F0) > 100 and np.array_equal(F0, F1) and V0.shape == V1.shape
    assert moved > 0   # predict refined: the flag and the images reached the stage
    assert cli.read_bytes() == plys["refined"].read_bytes()
    # the command line also refines a grid laid on the fixture's ground (normals towards the cameras) against the folder predict
    # wrote, and writes what refine_mesh gives in this process
    from deep3d_aerial_amd import ortho, refine

    xs, ys = np.linspace(-60.0, 200.0, 27), np.linspace(-60.0, 60.0, 13)
    gx, gy = np.meshgrid(xs, ys)
    G = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 500.0) + 3.0 * np.sin(gx.ravel() / 17.0)], 1).astype(np.float32)
    idx = np.arange(G.shape[0]).reshape(13, 27)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    GF = np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, d], 1)]).astype(np.int32)
    grid_in, grid_out = tmp_path / "grid" / "in.ply", tmp_path / "grid" / "out.ply"
    mesh.write_ply(str(grid_in), G, GF)
    gflags = ["--reach=3", "--spacing=4", "--min_score=-1", "--smooth_iterations=4", "--depth_tolerance=0.5", "--views_per_batch=2"]
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.refine", "--mesh", str(grid_in), "--mvs", str(tmp_path / "plain" / "MVS"),
                          "--out", str(grid_out), "--step", "5"] + gflags, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    want, info = refine.refine_mesh(torch.from_numpy(G).cuda(), torch.from_numpy(GF).cuda(), ortho.load_mvs_views(str(tmp_path / "plain" / "MVS")),
                                    5.0, reach=3, spacing=4.0, min_score=-1.0, smooth_iterations=4, depth_tolerance=0.5)
    print("grid: %s" % refine.summary_line(info))
    Vg, Fg = mesh.read_ply(str(grid_out))
    assert np.array_equal(Fg, GF) and _same(want, Vg)
    assert info["scales"][0]["active"] == 25 * 11 and info["scales"][0]["two_views"] > 0 and info["scales"][0]["moved"] > 0
    assert not np.array_equal(Vg, G)
