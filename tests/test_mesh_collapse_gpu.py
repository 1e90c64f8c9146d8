"""The kernel of csrc/mesh_collapse.hip and the driver of deep3d_aerial_amd/collapse.py on the GPU, bit for bit against the numpy
restatement of tests/test_mesh_collapse.py on the scene of tests/mesh_collapse_scene.py: measure, key, target, claim, winners, remap and
the mesh after one round, for any batching and view order; the loop against the chain of rounds; face permutations; empty meshes and
errors; the step off and the step before the subdivision in build_and_write; and the files written by predict, by the mesh tool,
by python -m deep3d_aerial_amd.collapse and on one and two ranks."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_collapse_scene as CS
import test_mesh_collapse as T

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


def _record(want, n, m):
    won = want["winners"] > 0
    return {"edges": len(want["edges"]), "short": want["short"], "valid": want["valid"], "winners": want["winners"],
            "vertices_out": len(want["vertices"]) if won else n, "faces_out": len(want["faces"]) if won else m}


def _check_round(got, want):
    """Every pass of collapse_round's detail against one round of the restatement."""
    assert got["n_edges"] == len(want["edges"]) and _same(got["edges"], want["edges"])
    assert _same(got["offset"], want["offset"]) and _same(got["nbr"], want["nbr"]) and _same(got["fixed"], want["fixed"])
    assert _same(got["face_offset"], want["face_offset"]) and _same(got["face_index"], want["face_index"])
    assert _same(got["measure"], want["measure"])
    assert _same(got["key"], want["key"]) and _same(got["target"], want["target"])
    assert _same(got["claim"], want["claim"]) and _same(got["win"], want["win"]) and _same(got["remap"], want["remap"])


@pytest.mark.parametrize("batch,reverse", [(None, False), (2, False), (None, True)])
def test_every_pass_of_a_round_is_bit_equal_to_numpy(batch, reverse):
    from deep3d_aerial_amd import collapse

    s = T.scene()
    want = s["detail"][0]
    v, f = _mesh(s["V"], s["F"])
    mv = _views(s["views"][::-1] if reverse else s["views"])
    detail = {}
    out_v, out_f, rec = collapse.collapse_round(v, f, mv, CS.MIN_EDGE, CS.MAX_EDGE, CS.TOLERANCE, batch, detail=detail)
    _check_round(detail, want)
    assert want["winners"] > 0 and _same(out_v, want["vertices"]) and _same(out_f, want["faces"])
    assert _same(v, s["V"]) and _same(f, s["F"])   # the inputs are read only
    assert rec == _record(want, len(s["V"]), len(s["F"]))
    # a later round, where the grid is the only piece still moving; and the last, which has no winner: the inputs come back
    for k in (7, len(s["detail"]) - 1):
        prev, want = s["detail"][k - 1], s["detail"][k]
        v, f = _mesh(prev["vertices"], prev["faces"])
        detail = {}
        out_v, out_f, rec = collapse.collapse_round(v, f, mv, CS.MIN_EDGE, CS.MAX_EDGE, CS.TOLERANCE, batch, detail=detail)
        _check_round(detail, want)
        assert rec == _record(want, len(prev["vertices"]), len(prev["faces"]))
        if want["winners"]:
            assert _same(out_v, want["vertices"]) and _same(out_f, want["faces"])
        else:
            assert out_v is v and out_f is f


def test_the_loop_equals_the_chain_of_rounds_and_the_numpy_loop():
    from deep3d_aerial_amd import collapse

    s = T.scene()
    v, f = _mesh(s["V"], s["F"])
    mv = _views(s["views"])
    info = {}
    out_v, out_f = collapse.collapse(v, f, mv, CS.MIN_EDGE, CS.MAX_EDGE, rounds=CS.ROUNDS, views_per_batch=3, info=info)
    assert _same(out_v, s["out_v"]) and _same(out_f, s["out_f"]) and info == s["info"]
    assert not info["hit_max_rounds"] and info["winners"][-1] == 0 and info["rounds"] == len(s["detail"])
    # the chain of rounds, each against the restatement's
    cv, cf = v, f
    for want in s["detail"]:
        n, m = int(cv.shape[0]), int(cf.shape[0])
        cv, cf, rec = collapse.collapse_round(cv, cf, mv, CS.MIN_EDGE, CS.MAX_EDGE)
        assert rec == _record(want, n, m)
    assert _same(cv, s["out_v"]) and _same(cf, s["out_f"])
    # the default max_edge is 4 min_edge; capped at three rounds the loop says so
    info = {}
    v3, f3 = collapse.collapse(v, f, mv, CS.MIN_EDGE, rounds=3, info=info)
    assert _same(v3, s["detail"][2]["vertices"]) and _same(f3, s["detail"][2]["faces"]) and info["hit_max_rounds"] and info["rounds"] == 3
    # at rest nothing moves: the input tensors come back
    info = {}
    again_v, again_f = collapse.collapse(out_v, out_f, mv, CS.MIN_EDGE, CS.MAX_EDGE, info=info)
    assert again_v is out_v and again_f is out_f and info["winners"] == [0] and info["faces_out"] == info["faces_in"] == len(s["out_f"])


def test_permuting_the_faces_gives_the_same_vertices_and_face_set():
    from deep3d_aerial_amd import collapse

    s = T.scene()
    perm = np.random.default_rng(17).permutation(len(s["F"]))
    v, f = _mesh(s["V"], s["F"][perm])
    info = {}
    out_v, out_f = collapse.collapse(v, f, _views(s["views"]), CS.MIN_EDGE, CS.MAX_EDGE, rounds=CS.ROUNDS, info=info)
    assert _same(out_v, s["out_v"]) and np.array_equal(T.S.canonical(out_f.cpu().numpy()), T.S.canonical(s["out_f"])) and info == s["info"]


def test_empty_meshes_cpu_tensors_and_bad_arguments():
    from deep3d_aerial_amd import _lib, collapse

    lib = _lib.load()
    t = torch.zeros((64,), dtype=torch.float64, device="cuda")
    o = torch.zeros((64,), dtype=torch.float64, device="cuda")
    p, q = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr())
    E = _lib.ERR_INVALID_ARG
    call = lambda vertices=p, n=4, m=1, emax=3, lo=1.0, hi=4.0, key=q: lib.d3d_mesh_collapse_candidates(
        vertices, n, p, m, p, p, p, p, p, p, p, emax, p, lo, hi, q, key, None)
    assert call(emax=0) == 0 and call(n=0, m=0, emax=0) == 0   # nothing to launch
    assert call(vertices=None) == E and call(key=None) == E
    assert b"null pointer" in lib.d3d_last_error()
    assert call(n=1 << 31) == E and call(n=-1) == E and call(m=(1 << 31) // 6 + 1) == E and call(m=-1) == E
    assert call(emax=1 << 31) == E and call(emax=-1) == E
    for lo in (0.0, -1.0, float("nan"), float("inf")):
        assert call(lo=lo) == E
    assert b"min_edge" in lib.d3d_last_error()
    for hi in (1.5, float("nan"), float("inf")):
        assert call(hi=hi) == E
    assert b"max_edge" in lib.d3d_last_error()
    torch.cuda.synchronize()
    assert not t.any() and not o.any()
    # the Python side: empty meshes come back as they are, settings are checked before anything runs
    mv = _views(T.scene()["views"][:2])
    v0, f0 = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    info = {}
    out = collapse.collapse(v0, f0, mv, 1.0, info=info)
    assert out[0] is v0 and out[1] is f0
    assert info == {"edges": [], "short": [], "valid": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces_in": 0, "faces_out": 0,
                    "vertices_out": 0}
    v, f = _mesh(*T.S.grid(3, 3))
    out = collapse.collapse(v, f0, mv, 1.0)
    assert out[0] is v and out[1] is f0
    rv, rf, rec = collapse.collapse_round(v, f0, mv, 1.0, 4.0)
    assert rv is v and rf is f0 and rec == {"edges": 0, "short": 0, "valid": 0, "winners": 0, "vertices_out": 9, "faces_out": 0}
    for bad in ({"min_edge": 0}, {"min_edge": 1, "max_edge": 1.5}, {"min_edge": 1, "rounds": 0}, {"min_edge": 1, "rounds": 65},
                {"min_edge": 1, "depth_tolerance": -1}, {"min_edge": 1, "views_per_batch": 0}):
        with pytest.raises(ValueError):
            collapse.collapse(v, f, mv, **bad)
    with pytest.raises(TypeError):
        collapse.collapse(v, f, [object()], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        collapse.collapse(v.cpu(), f.cpu(), [], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        collapse.collapse_round(v.cpu(), f.cpu(), [], 1.0, 4.0)


def test_a_face_with_a_repeated_index_is_refused_only_when_the_step_is_on(tmp_path, monkeypatch):
    from deep3d_aerial_amd import collapse, mesh

    s = T.scene()
    v, f = _mesh(s["V"], s["F"])
    bad = f.clone()
    bad[3, 1] = bad[3, 0]
    mv = _views(s["views"][:2])
    with pytest.raises(ValueError, match="repeated index"):
        collapse.collapse(v, bad, mv, CS.MIN_EDGE)
    with pytest.raises(ValueError, match="repeated index"):
        collapse.collapse_round(v, bad, mv, CS.MIN_EDGE, CS.MAX_EDGE)
    # build_and_write with the step off never looks: the mesh stage's own output goes through as it does today
    monkeypatch.setattr(mesh, "depth_to_mesh", lambda *a, **k: (v, bad))
    settings = {"path": str(tmp_path / "off.ply"), "border": [0, 1, 0, 1, 0, 1], "voxel": 0.5}
    got = mesh.build_and_write(mv, settings)
    assert got[0] is v and got[1] is bad
    with pytest.raises(ValueError, match="repeated index"):
        mesh.build_and_write(mv, dict(settings, collapse={"min_edge": CS.MIN_EDGE}))


def test_the_step_off_returns_the_tensors_the_mesh_stage_returns(tmp_path, monkeypatch):
    import mesh_scene as MS
    import texture_scene as TS
    from deep3d_aerial_amd import collapse, mesh

    scene = CS.PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    mv = _views(scene.views)
    want_v, want_f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel), None, 2, 0.2, None)
    called = []
    real = collapse.collapse
    monkeypatch.setattr(collapse, "collapse", lambda *a, **k: called.append(1) or real(*a, **k))
    settings = MS.pipeline_settings(str(tmp_path / "off.ply"), border, voxel)
    v, f = mesh.build_and_write(mv, settings)
    assert not called and _same(v, want_v.cpu().numpy()) and _same(f, want_f.cpu().numpy())
    # an unrelated key changes nothing either
    tm = {}
    v1, f1 = mesh.build_and_write(mv, dict(settings, path=str(tmp_path / "other.ply"), decimate_max_rounds=7), timings=tm)
    assert not called and "mesh_collapse_s" not in tm and _same(v1, v.cpu().numpy()) and _same(f1, f.cpu().numpy())
    mesh.write_ply(str(tmp_path / "want.ply"), want_v, want_f)
    assert (tmp_path / "off.ply").read_bytes() == (tmp_path / "want.ply").read_bytes() == (tmp_path / "other.ply").read_bytes()
    # on: the same mesh, collapsed against the same views
    v2, f2 = mesh.build_and_write(mv, dict(settings, path=str(tmp_path / "on.ply"), collapse={"min_edge": 1.0, "rounds": 4}), timings=tm)
    info = {}
    cv, cf = real(want_v, want_f, mv, 1.0, rounds=4, info=info)
    print("mesh stage: %d faces; %s" % (want_f.shape[0], collapse.summary_line(info)))
    assert called and tm["mesh_collapse_s"] > 0 and info["winners"][0] > 0
    assert _same(v2, cv.cpu().numpy()) and _same(f2, cf.cpu().numpy()) and f2.shape[0] < f.shape[0]
    V, F = mesh.read_ply(str(tmp_path / "on.ply"))
    assert _same(cv, V) and _same(cf, F)


def test_collapse_then_subdivision_is_the_composition_of_the_two(tmp_path):
    import mesh_scene as MS
    import texture_scene as TS
    from deep3d_aerial_amd import collapse, mesh, subdivide

    scene = CS.PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    mv = _views(scene.views)
    v, f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel), None, 2, 0.2, None)
    settings = dict(MS.pipeline_settings(str(tmp_path / "both.ply"), border, voxel), collapse={"min_edge": 1.0, "rounds": 4},
                    subdivide={"max_edge": 2.0, "rounds": 1})
    assert mesh.collapse_settings(settings)["max_edge"] == 2.0   # the subdivision's, exactly 2 min_edge
    tm = {}
    got_v, got_f = mesh.build_and_write(mv, settings, timings=tm)
    ci, si = {}, {}
    cv, cf = collapse.collapse(v, f, mv, 1.0, max_edge=2.0, rounds=4, info=ci)
    sv, sf = subdivide.subdivide(cv, cf, mv, 2.0, rounds=1, info=si)
    assert ci["winners"][0] > 0 and si["rounds"][0]["split"] > 0 and tm["mesh_collapse_s"] > 0 and tm["mesh_subdivide_s"] > 0
    assert _same(got_v, sv.cpu().numpy()) and _same(got_f, sf.cpu().numpy())
    with pytest.raises(ValueError, match="2 min_edge"):
        mesh.build_and_write(mv, dict(settings, collapse={"min_edge": 1.5}))


# ----------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


def _launch(n_ranks, out_dir, border, voxel, min_edge):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mesh_collapse_scene.py"), str(out_dir),
           ",".join(repr(b) for b in border), repr(voxel), repr(min_edge)]
    res = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_collapsed_mesh_one_rank_writes(tmp_path):
    import texture_scene as TS
    from deep3d_aerial_amd import collapse, mesh

    scene = CS.PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    out1 = _launch(1, tmp_path / "one", border, voxel, 1.0)
    out2 = _launch(2, tmp_path / "two", border, voxel, 1.0)
    assert "rank 0/1 mesh_collapse" in out1 and "rank 0/2 mesh_collapse" in out2 and "rank 1/2" in out2
    assert (tmp_path / "one" / "mesh.ply").read_bytes() == (tmp_path / "two" / "mesh.ply").read_bytes()
    # it is the mesh stage's mesh, collapsed
    mv = _views(scene.views)
    v, f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel))
    want_v, want_f = collapse.collapse(v, f, mv, 1.0, rounds=4)
    V, F = mesh.read_ply(str(tmp_path / "one" / "mesh.ply"))
    assert len(F) < f.shape[0] and _same(want_v, V) and _same(want_f, F)


def test_predict_the_mesh_tool_and_the_standalone_tool_write_the_same_mesh(tmp_path):
    """predict --fuse --mesh on the block fixture (seeded casmvsnet weights: plumbing, not geometry) without the flag and with
    --mesh_collapse 1; python -m deep3d_aerial_amd.mesh --mvs ... --collapse 1 on the MVS folder predict wrote; python -m
    deep3d_aerial_amd.collapse on the plain mesh and that folder.  The three collapsed files are byte for byte the same, and they
    hold what collapse() gives in this process."""
    import block_fixture as BF
    from deep3d_aerial_amd import collapse, mesh, mvs_dl, predict as P, synthetic as Sy

    folder = BF.write_block(str(tmp_path / "block"))
    model = P.build_model("casmvsnet", BF.NUM_DEPTH)
    Sy.fill_state_dict_(model.state_dict(), 31)
    ckpt = str(tmp_path / "model_000001_0.1000.ckpt")
    torch.save({"epoch": 1, "model": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, ckpt)
    flags = ["--border=-200,400,-200,200,400,600", "--voxel=10", "--min_views=1", "--conf_threshold=0"]
    plys = {}
    for name, extra in (("plain", []), ("on", ["--mesh_collapse", "1"])):
        plys[name] = tmp_path / name / "block.ply"
        mvs_dl.MVS_Inference(BF.MAX_W, BF.MAX_H, view_num=BF.VIEW_NUM, num_depth=BF.NUM_DEPTH, model_type="casmvsnet", pretrain_weight=ckpt,
                             extra_args=["--fuse", "--fuse_filter_sources=0", "--geo_consist_num=1", "--depth_threshold=0.5",
                                         "--position_threshold=50", "--mesh", str(plys[name])] + ["--mesh_" + f[2:] for f in flags] +
                             extra).run(folder, str(tmp_path / name / "MVS"))
    mvs = str(tmp_path / "plain" / "MVS")
    tool, cli = tmp_path / "tool" / "block.ply", tmp_path / "cli" / "block.ply"
    os.makedirs(str(tmp_path / "tool"))
    os.makedirs(str(tmp_path / "cli"))
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.mesh", "--mvs", mvs, "--out", str(tool), "--collapse", "1"] + flags, cwd=ROOT,
                         env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "mesh collapse:" in res.stdout
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.collapse", "--mesh", str(plys["plain"]), "--mvs", mvs, "--out", str(cli),
                          "--min_edge", "1"], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "collapsed mesh" in res.stdout
    assert plys["on"].read_bytes() == tool.read_bytes() == cli.read_bytes() != plys["plain"].read_bytes()
    V0, F0 = mesh.read_ply(str(plys["plain"]))
    info = {}
    cv, cf = collapse.collapse(torch.from_numpy(V0).cuda(), torch.from_numpy(F0).cuda(), mesh.load_mvs_views(mvs), 1.0, info=info)
    print("block: %d vertices, %d faces; %s" % (len(V0), len(F0), collapse.summary_line(info)))
    Vc, Fc = mesh.read_ply(str(cli))
    assert len(F0) > 100 and info["winners"][0] > 0 and len(Fc) < len(F0) and _same(cv, Vc) and _same(cf, Fc)
