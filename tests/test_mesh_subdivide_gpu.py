"""The kernels of csrc/mesh_subdivide.hip on the GPU, bit for bit against the numpy restatement of tests/test_mesh_subdivide.py on the
scene of tests/mesh_subdivide_scene.py: the measure (batching, order, halves), marks, new indices, midpoints, per-face edge indices,
child counts and offsets, totals and the emitted mesh, for one round and for the loop; scans past one tile; errors; the step off;
and the files written by predict, by python -m deep3d_aerial_amd.subdivide and on one and two ranks."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_subdivide_scene as SS
import test_mesh_subdivide as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _views(vs):
    from deep3d_aerial_amd import mesh

    return [mesh.MeshView(v["K"], v["E"], torch.from_numpy(np.ascontiguousarray(v["depth"], np.float32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(v.get("confidence", np.ones_like(v["depth"])), np.float32)).cuda()) for v in vs]


def _mesh(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F, np.int32)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.shape == np.asarray(want).shape and np.array_equal(_bits(got), _bits(want))


def _check_round(got, want):
    """Every pass of subdivide_round's detail against one round of the restatement."""
    assert got["n_edges"] == len(want["edges"]) and _same(got["edges"], want["edges"])
    assert _same(got["measure"], want["measure"])
    assert _same(got["mark"], want["mark"]) and _same(got["rank"], want["rank"]) and _same(got["midpoint"], want["midpoint"])
    assert _same(got["face_edge"], want["face_edge"])
    assert _same(got["child_count"], want["child_count"]) and _same(got["child_offset"], want["child_offset"])
    assert got["totals"].cpu().tolist() == want["totals"].tolist()


@pytest.mark.parametrize("batch,reverse", [(None, False), (2, False), (None, True)])
def test_every_pass_is_bit_equal_to_numpy(batch, reverse):
    from deep3d_aerial_amd import subdivide

    s = T.scene()
    want = s["detail"][0]
    v, f = _mesh(s["V"], s["F"])
    mv = _views(s["views"][::-1] if reverse else s["views"])
    detail = {}
    out_v, out_f, rec = subdivide.subdivide_round(v, f, mv, SS.MAX_EDGE, SS.TOLERANCE, batch, detail=detail)
    _check_round(detail, want)
    assert _same(out_v, want["out_v"]) and _same(out_f, want["out_f"])
    assert _same(v, s["V"]) and _same(f, s["F"])   # the inputs are read only
    assert rec == {"edges": len(want["edges"]), "seen": int((want["measure"] > 0).sum()), "split": int(want["totals"][0]),
                   "vertices_out": len(want["out_v"]), "faces_out": len(want["out_f"]), "longest_px": float(np.sqrt(want["measure"].max()))}
    assert _same(out_v[:len(s["V"])], s["V"])   # the input vertices come first, unchanged


def test_two_halves_of_the_views_max_merge_to_the_whole_measure():
    from deep3d_aerial_amd import subdivide

    s = T.scene()
    want = s["detail"][0]
    v, f = _mesh(s["V"], s["F"])
    mv = _views(s["views"])
    edges, n_edges = subdivide.edge_list(f, int(v.shape[0]))
    ne = int(n_edges.item())
    assert ne == len(want["edges"]) and edges.shape[0] == 3 * len(s["F"])
    half = subdivide.measure_edges(v, edges, n_edges, mv[4:], SS.TOLERANCE)
    assert _same(half[:ne], T.measure_numpy(s["V"], want["edges"], s["views"][4:])) and not _same(half[:ne], want["measure"])
    both = subdivide.measure_edges(v, edges, n_edges, mv[:4], SS.TOLERANCE, measure=half)
    assert both is half and _same(both[:ne], want["measure"]) and not both[ne:].any()
    again = subdivide.measure_edges(v, edges, n_edges, mv, SS.TOLERANCE, views_per_batch=3, measure=both.clone())
    assert _same(again[:ne], want["measure"])
    assert not subdivide.measure_edges(v, edges, n_edges, [], SS.TOLERANCE).any()
    # the plan from the merged measure is the round's
    p = subdivide.plan(v, f, edges, n_edges, both, SS.MAX_EDGE)
    assert _same(p["mark"][:ne], want["mark"]) and p["totals"].cpu().tolist() == want["totals"].tolist() and not p["mark"][ne:].any()


def test_one_round_and_the_full_loop_equal_the_chain():
    from deep3d_aerial_amd import subdivide

    s, c = T.scene(), T.core()
    v, f = _mesh(s["V"], s["F"])
    mv = _views(s["views"])
    info = {}
    v1, f1 = subdivide.subdivide(v, f, mv, SS.MAX_EDGE, rounds=1, info=info)
    assert _same(v1, s["detail"][0]["out_v"]) and _same(f1, s["detail"][0]["out_f"]) and len(info["rounds"]) == 1 and not info["stopped_early"]
    info = {}
    vo, fo = subdivide.subdivide(v, f, mv, SS.MAX_EDGE, views_per_batch=3, info=info)
    assert _same(vo, s["out_v"]) and _same(fo, s["out_f"])
    assert [r["split"] for r in info["rounds"]] == [int(d["totals"][0]) for d in s["detail"]] and not info["stopped_early"]
    assert info["vertices"] == len(s["out_v"]) and info["faces"] == len(s["out_f"])
    # the core comes to rest: the loop stops early, and its last round emits nothing
    info = {}
    fc = torch.from_numpy(c["F"]).cuda()
    vo, fo = subdivide.subdivide(v, fc, mv, SS.MAX_EDGE, info=info)
    assert _same(vo, c["out_v"]) and _same(fo, c["out_f"]) and info["stopped_early"] and len(info["rounds"]) == len(c["detail"])
    assert info["rounds"][-1]["split"] == 0 and info["rounds"][-1]["faces_out"] == len(c["out_f"])
    again_v, again_f = subdivide.subdivide(vo, fo, mv, SS.MAX_EDGE)
    assert again_v is vo and again_f is fo   # nothing to split: the input tensors come back


def test_splits_and_faces_are_numbered_by_scans_past_one_tile():
    """A 48 x 48 grid under one camera that sees every edge longer than the limit: 6721 split edges and 4418 faces, both more than
    one scan tile of 4096 values."""
    from deep3d_aerial_amd import subdivide

    V, F = T.grid(48, 48, step=1.0, z=10.0)
    view = T.flat_view(f=100.0, size=601, depth=10.0, centre=(23.5, 23.5))
    detail = []
    want_v, want_f, _ = T.subdivide_numpy(V, F, [view], 4.0, rounds=1, detail=detail)
    assert detail[0]["totals"].tolist() == [len(detail[0]["edges"]), 4 * len(F)] and detail[0]["totals"][0] > 4096 and len(F) > 4096
    got = {}
    v, f = _mesh(V, F)
    out_v, out_f, rec = subdivide.subdivide_round(v, f, _views([view]), 4.0, detail=got)
    _check_round(got, detail[0])
    assert _same(out_v, want_v) and _same(out_f, want_f)


def test_empty_meshes_bad_arguments_and_the_int32_refusal():
    from deep3d_aerial_amd import _lib, subdivide

    lib = _lib.load()
    t = torch.zeros((64,), dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    E = _lib.ERR_INVALID_ARG
    # n = 0 and m = 0 are fine and launch nothing that writes past the arrays
    assert lib.d3d_mesh_subdivide_measure(p, 0, p, p, 0, p, 0, 0.01, p, None) == 0
    nbytes = lib.d3d_mesh_subdivide_scratch_bytes(0, 0)
    assert nbytes > 0 and lib.d3d_mesh_subdivide_scratch_bytes(-1, 0) == 0 and lib.d3d_mesh_subdivide_scratch_bytes(0, 1 << 31) == 0
    assert lib.d3d_mesh_subdivide_scratch_bytes(((1 << 31) - 1) // 6 + 1, 0) == 0
    scratch = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    sp, tp = ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(totals.data_ptr())
    assert lib.d3d_mesh_subdivide_plan(p, 0, p, 0, p, p, 0, p, 4.0, sp, nbytes, p, p, p, p, p, p, tp, None) == 0
    assert totals.cpu().tolist() == [0, 0]
    o = torch.zeros((64,), dtype=torch.float64, device="cuda")
    q = ctypes.c_void_p(o.data_ptr())
    assert lib.d3d_mesh_subdivide_emit(p, 0, p, 0, p, 0, p, p, p, p, p, 0, 0, q, q, None) == 0
    # bad arguments and their error code
    assert lib.d3d_mesh_subdivide_measure(None, 4, p, p, 4, p, 1, 0.01, p, None) == E
    assert lib.d3d_mesh_subdivide_measure(p, 4, p, p, 4, p, 1, -0.5, p, None) == E
    assert lib.d3d_mesh_subdivide_measure(p, 4, p, p, 4, p, 1, float("nan"), p, None) == E
    assert lib.d3d_mesh_subdivide_measure(p, 4, p, p, 1 << 31, p, 1, 0.01, p, None) == E
    assert lib.d3d_mesh_subdivide_measure(p, 4, p, p, 4, p, 1 << 20, 0.01, p, None) == E
    assert lib.d3d_mesh_subdivide_measure(p, 4, p, p, 4, p, -1, 0.01, p, None) == E
    assert lib.d3d_mesh_subdivide_plan(p, 4, p, 1, p, p, 3, p, 0.5, sp, nbytes, p, p, p, p, p, p, tp, None) == E
    assert lib.d3d_mesh_subdivide_plan(p, 4, p, 1, p, p, 3, p, float("inf"), sp, nbytes, p, p, p, p, p, p, tp, None) == E
    assert lib.d3d_mesh_subdivide_plan(p, 4, p, 1, p, p, 3, p, 4.0, sp, 8, p, p, p, p, p, p, tp, None) == E
    assert lib.d3d_mesh_subdivide_plan(p, 4, p, 1, p, p, 3, p, 4.0, sp, nbytes, p, p, p, p, p, p, None, None) == E
    assert lib.d3d_mesh_subdivide_plan(p, 4, p, (1 << 31) // 6 + 1, p, p, 3, p, 4.0, sp, nbytes, p, p, p, p, p, p, tp, None) == E
    assert lib.d3d_mesh_subdivide_emit(p, 4, p, 1, p, 3, p, p, p, p, p, 1, 2, p, q, None) == E        # the outputs are the inputs
    assert lib.d3d_mesh_subdivide_emit(p, 4, p, 1, p, 3, p, p, p, p, p, 4, 2, q, q, None) == E        # more splits than edges
    assert lib.d3d_mesh_subdivide_emit(p, 4, p, 1, p, 3, p, p, p, p, p, 1, 5, q, q, None) == E        # more than four children a face
    assert lib.d3d_mesh_subdivide_emit(p, (1 << 31) - 2, p, 1, p, 3, p, p, p, p, p, 2, 2, q, q, None) == E   # n + splits reaches 2^31
    assert b"n_split" in lib.d3d_last_error()
    torch.cuda.synchronize()
    assert not t.any() and not o.any()
    # the Python side: empty meshes come back as they are, settings are checked before anything runs
    mv = _views(T.scene()["views"][:2])
    v0, f0 = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    info = {}
    assert subdivide.subdivide(v0, f0, mv, 4.0, info=info)[0] is v0 and info == {"rounds": [], "stopped_early": False, "vertices": 0, "faces": 0}
    v, f = _mesh(*T.grid(3, 3))
    out = subdivide.subdivide(v, f0, mv, 4.0)
    assert out[0] is v and out[1] is f0
    for bad in ({"max_edge": 0.5}, {"max_edge": 4, "rounds": 0}, {"max_edge": 4, "rounds": 9}, {"max_edge": 4, "depth_tolerance": -1},
                {"max_edge": 4, "views_per_batch": 0}):
        with pytest.raises(ValueError):
            subdivide.subdivide(v, f, mv, **bad)
    with pytest.raises(TypeError):
        subdivide.subdivide(v, f, [object()], 4.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        subdivide.subdivide(v.cpu(), f.cpu(), [], 4.0)
    # the int32 refusal, through the size check alone: emit refuses before it allocates
    with pytest.raises(ValueError, match="int32"):
        subdivide.emit(v, f, None, {}, (1 << 31) - int(v.shape[0]), 4 * int(f.shape[0]))
    with pytest.raises(ValueError, match="int32"):
        subdivide.emit(v, f, None, {}, 1, (1 << 31) // 6 + 1)


def test_a_face_with_a_repeated_index_is_refused_only_when_the_step_is_on(tmp_path, monkeypatch):
    from deep3d_aerial_amd import mesh, subdivide

    s = T.scene()
    v, f = _mesh(s["V"], s["F"])
    bad = f.clone()
    bad[3, 1] = bad[3, 0]
    mv = _views(s["views"][:2])
    with pytest.raises(ValueError, match="repeated index"):
        subdivide.subdivide(v, bad, mv, SS.MAX_EDGE)
    with pytest.raises(ValueError, match="repeated index"):
        subdivide.subdivide_round(v, bad, mv, SS.MAX_EDGE)
    # build_and_write with the step off never looks: the mesh stage's own output goes through as it does today
    monkeypatch.setattr(mesh, "depth_to_mesh", lambda *a, **k: (v, bad))
    settings = {"path": str(tmp_path / "off.ply"), "border": [0, 1, 0, 1, 0, 1], "voxel": 0.5}
    got = mesh.build_and_write(mv, settings)
    assert got[0] is v and got[1] is bad
    with pytest.raises(ValueError, match="repeated index"):
        mesh.build_and_write(mv, dict(settings, subdivide={"max_edge": SS.MAX_EDGE}))


def test_the_step_off_returns_the_tensors_the_mesh_stage_returns(tmp_path, monkeypatch):
    import mesh_scene as MS
    import texture_scene as TS
    from deep3d_aerial_amd import mesh, subdivide

    scene = SS.PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    mv = _views(scene.views)
    want_v, want_f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel), None, 2, 0.2, None)
    called = []
    real = subdivide.subdivide
    monkeypatch.setattr(subdivide, "subdivide", lambda *a, **k: called.append(1) or real(*a, **k))
    settings = MS.pipeline_settings(str(tmp_path / "off.ply"), border, voxel)
    v, f = mesh.build_and_write(mv, settings)
    assert not called and _same(v, want_v.cpu().numpy()) and _same(f, want_f.cpu().numpy())
    mesh.write_ply(str(tmp_path / "want.ply"), want_v, want_f)
    assert (tmp_path / "off.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    # on: the same mesh, subdivided against the same views
    tm = {}
    v2, f2 = mesh.build_and_write(mv, dict(settings, path=str(tmp_path / "on.ply"), subdivide={"max_edge": 1.0, "rounds": 1}), timings=tm)
    info = {}
    sv, sf = real(want_v, want_f, mv, 1.0, rounds=1, info=info)
    assert called and tm["mesh_subdivide_s"] > 0 and info["rounds"][0]["split"] > 100
    assert _same(v2, sv.cpu().numpy()) and _same(f2, sf.cpu().numpy()) and f2.shape[0] > f.shape[0]
    V, F = mesh.read_ply(str(tmp_path / "on.ply"))
    assert _same(sv, V) and _same(sf, F)


# ----------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def _launch(n_ranks, out_dir, border, voxel, max_edge):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mesh_subdivide_scene.py"), str(out_dir),
           ",".join(repr(b) for b in border), repr(voxel), repr(max_edge)]
    res = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_subdivided_mesh_one_rank_writes(tmp_path):
    import texture_scene as TS
    from deep3d_aerial_amd import mesh, subdivide

    scene = SS.PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    out1 = _launch(1, tmp_path / "one", border, voxel, 1.0)
    out2 = _launch(2, tmp_path / "two", border, voxel, 1.0)
    assert "rank 0/1 mesh_subdivide" in out1 and "rank 0/2 mesh_subdivide" in out2 and "rank 1/2" in out2
    assert (tmp_path / "one" / "mesh.ply").read_bytes() == (tmp_path / "two" / "mesh.ply").read_bytes()
    # it is the mesh stage's mesh, subdivided
    mv = _views(scene.views)
    v, f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel))
    want_v, want_f = subdivide.subdivide(v, f, mv, 1.0, rounds=2)
    V, F = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    assert len(F) > 2 * f.shape[0] and _same(want_v, V) and _same(want_f, F)


def test_predict_the_standalone_tool_and_subdivide_write_the_same_mesh(tmp_path):
    """predict --fuse --mesh on the block fixture (seeded casmvsnet weights: plumbing, not geometry) without the flag, and with
    --mesh_subdivide, the refinement, the DSM from the mesh and the texture behind it; python -m deep3d_aerial_amd.subdivide on the
    plain mesh and the MVS folder predict wrote.  Without the flag the PLY is the mesh stage's own; the tool writes what subdivide()
    gives in this process; predict's mesh is that mesh refined, and the DSM and the texture are made from it."""
    import argparse

    import block_fixture as BF
    from deep3d_aerial_amd import mesh, mvs_dl, ortho, predict as P, refine, subdivide, synthetic as Sy, texture

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    Sy.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    flags = ["--border=-200,400,-200,200,400,600", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    rflags = ["--reach=3", "--spacing=4", "--min_score=-1", "--smooth_iterations=4"]
    tex, dsm = tmp_path / "full" / "tex" / "block.ply", tmp_path / "full" / "dsm.tif"
    full = ["--mesh_subdivide", "1", "--mesh_subdivide_rounds", "2", "--mesh_refine", "5"] + ["--mesh_refine_" + r[2:] for r in rflags] + \
           ["--dsm", str(dsm), "--dsm_border=-200,400,-200,200", "--dsm_unit=5,5", "--dsm_source", "mesh",
            "--texture", str(tex), "--texture_depth_tolerance=0.5", "--texture_page_size=256"]
    plys = {}
    for name, extra in (("plain", []), ("full", full)):
        plys[name] = tmp_path / name / "block.ply"
        mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                             extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                         "--position_threshold=50", "--mesh", str(plys[name])] + ["--mesh_" + f[2:] for f in flags] +
                             extra).run(folder, str(tmp_path / name / "MVS"))
    # off: the mesh stage's own file
    ap = argparse.ArgumentParser()
    mesh.add_arguments(ap)
    direct = tmp_path / "direct" / "block.ply"
    mvs = str(tmp_path / "plain" / "MVS")
    mesh.build_and_write(mesh.load_mvs_views(mvs), mesh.settings_from_args(ap.parse_args(flags), str(direct)))
    assert direct.read_bytes() == plys["plain"].read_bytes()
    # the stand-alone tool against subdivide() in this process
    cli = tmp_path / "cli" / "block.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.subdivide", "--mesh", str(plys["plain"]), "--mvs", mvs, "--out", str(cli),
                          "--max_edge", "1", "--rounds", "2"], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "subdivided mesh" in res.stdout
    V0, F0 = mesh.read_ply(str(plys["plain"]))
    info = {}
    sv, sf = subdivide.subdivide(torch.from_numpy(V0).cuda(), torch.from_numpy(F0).cuda(), mesh.load_mvs_views(mvs), 1.0, rounds=2, info=info)
    print("block: %d vertices, %d faces; %s" % (len(V0), len(F0), subdivide.summary_line(info)))
    Vc, Fc = mesh.read_ply(str(cli))
    assert len(F0) > 100 and info["rounds"][0]["split"] > 0 and len(Fc) > len(F0)
    assert _same(sv, Vc) and _same(sf, Fc) and _same(sv[:len(V0)], V0)
    # the same flags through the mesh tool
    tool = tmp_path / "tool" / "block.ply"
    a = ap.parse_args(flags + ["--subdivide", "1", "--subdivide_rounds", "2"])
    mesh.build_and_write(mesh.load_mvs_views(mvs), mesh.settings_from_args(a, str(tool)))
    assert tool.read_bytes() == cli.read_bytes()
    # predict: that mesh, then refined; the DSM and the texture are made from it
    V1, F1 = mesh.read_ply(str(plys["full"]))
    assert np.array_equal(F1, Fc) and V1.shape == Vc.shape and not np.array_equal(V1, Vc)
    want, _ = refine.refine_mesh(sv, sf, ortho.load_mvs_views(str(tmp_path / "full" / "MVS")), 5.0, reach=3, spacing=4.0, min_score=-1.0,
                                 smooth_iterations=4)
    assert _same(want, V1)
    Vt, Ft, tc, tn, files = texture.read_textured_ply(str(tex))
    assert files and np.array_equal(Ft, F1) and _same(Vt, V1)
    assert dsm.exists() and dsm.stat().st_size > 0
