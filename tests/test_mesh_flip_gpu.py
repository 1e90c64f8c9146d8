"""The kernels of csrc/mesh_flip.hip and the driver of deep3d_aerial_amd/flip.py on the GPU, bit for bit against the numpy
restatement of tests/mesh_flip_scene.py on its scene: key, opp, claim, winners and faces of every round of the chain, the final
mesh, two runs, face permutations and corner rotations; empty meshes, refused inputs and the C entry points' argument checks; the
step in build_and_write, off, on, and between the collapse and the subdivision; and the files the mesh tool and python -m
deep3d_aerial_amd.flip write."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_flip_scene as FS
import test_mesh_flip as T

pytestmark = pytest.mark.gpu


def _mesh(V, F):
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F, np.int32)).cuda()


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _check_round(got, want):
    """Every pass of flip_round's detail against one round of the restatement."""
    assert got["n_edges"] == len(want["edges"]) and _same(got["edges"], want["edges"])
    assert _same(got["offset"], want["offset"]) and _same(got["nbr"], want["nbr"]) and _same(got["fixed"], want["fixed"])
    assert _same(got["face_offset"], want["face_offset"]) and _same(got["face_index"], want["face_index"])
    assert _same(got["key"], want["key"]) and _same(got["opp"], want["opp"])
    assert _same(got["claim"], want["claim"]) and _same(got["win"], want["win"])


def test_every_round_of_the_chain_is_bit_equal_to_numpy():
    from deep3d_aerial_amd import flip

    s = T.scene()
    v, f = _mesh(s["V"], s["F"])
    cf = f
    for want in s["detail"]:
        detail = {}
        before = cf
        out_v, cf, rec = flip.flip_round(v, cf, FS.MAX_ANGLE, detail=detail)
        _check_round(detail, want)
        assert rec == {"edges": len(want["edges"]), "candidates": want["candidates"], "winners": want["winners"]}
        assert out_v is v and _same(cf, want["faces"])
        if want["winners"] == 0:
            assert cf is before   # the input tensors come back
    assert _same(cf, s["out_f"]) and _same(f, s["F"]) and _same(v, s["V"])   # the inputs are read only


def test_the_loop_equals_the_numpy_loop_twice_and_capped():
    from deep3d_aerial_amd import flip

    s = T.scene()
    v, f = _mesh(s["V"], s["F"])
    info = {}
    out_v, out_f = flip.flip_edges(v, f, FS.MAX_ANGLE, rounds=FS.ROUNDS, info=info)
    assert out_v is v and _same(out_f, s["out_f"]) and info == s["info"]
    assert not info["hit_max_rounds"] and info["winners"][-1] == 0 and info["candidates"][-1] == 0
    # a second run gives the same bits, whatever order the atomics landed in
    again = {}
    v2, f2 = flip.flip_edges(v, f, FS.MAX_ANGLE, info=again)
    assert torch.equal(f2, out_f) and again == info
    # capped at three rounds the loop says so
    info3 = {}
    v3, f3 = flip.flip_edges(v, f, FS.MAX_ANGLE, rounds=3, info=info3)
    assert _same(f3, s["detail"][2]["faces"]) and info3["hit_max_rounds"] and info3["rounds"] == 3
    # at rest nothing flips: the input tensors come back
    rest = {}
    rv, rf = flip.flip_edges(v, out_f, FS.MAX_ANGLE, info=rest)
    assert rv is v and rf is out_f and rest["winners"] == [0] and rest["candidates"] == [0] and rest["flips"] == 0


def test_face_permutations_and_corner_rotations_give_the_same_face_set():
    from deep3d_aerial_amd import flip

    s = T.scene()
    want = T.S.canonical(s["out_f"])
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(s["F"]))
    turn = rng.integers(0, 3, len(s["F"]))
    rolled = np.stack([s["F"][np.arange(len(turn)), (turn + i) % 3] for i in range(3)], 1)
    for faces in (s["F"][perm], rolled, rolled[perm]):
        v, f = _mesh(s["V"], faces)
        info = {}
        out_v, out_f = flip.flip_edges(v, f, FS.MAX_ANGLE, info=info)
        assert np.array_equal(T.S.canonical(out_f.cpu().numpy()), want) and info == s["info"]


def test_empty_meshes_meshes_at_rest_and_refused_inputs():
    from deep3d_aerial_amd import flip

    v0, f0 = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    info = {}
    out = flip.flip_edges(v0, f0, 30.0, info=info)
    assert out[0] is v0 and out[1] is f0
    assert info == {"edges": [], "candidates": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces": 0, "flips": 0}
    v, f = _mesh(*T.S.grid(3, 3))
    out = flip.flip_edges(v, f0, 30.0)
    assert out[0] is v and out[1] is f0
    rv, rf, rec = flip.flip_round(v, f0, 30.0)
    assert rv is v and rf is f0 and rec == {"edges": 0, "candidates": 0, "winners": 0}
    # a regular grid has nothing to flip
    info = {}
    out = flip.flip_edges(v, f, 30.0, info=info)
    assert out[0] is v and out[1] is f and info["rounds"] == 1 and info["edges"] == [16] and info["candidates"] == [0]
    # refused, as the collapse refuses them
    bad = f.clone()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ValueError, match="repeated index"):
        flip.flip_edges(v, bad, 30.0)
    with pytest.raises(ValueError, match="repeated index"):
        flip.flip_round(v, bad, 30.0)
    for i in (9, -1):
        bad = f.clone()
        bad[2, 2] = i
        with pytest.raises(ValueError, match="outside"):
            flip.flip_edges(v, bad, 30.0)
    with pytest.raises(ValueError, match="int32"):
        flip.flip_edges(v, f.long(), 30.0)
    with pytest.raises(ValueError, match="float32"):
        flip.flip_edges(v.double(), f, 30.0)
    with pytest.raises(TypeError):
        flip.flip_edges(v.cpu().numpy(), f, 30.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flip.flip_edges(v.cpu(), f.cpu(), 30.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flip.flip_round(v.cpu(), f.cpu(), 30.0)
    for bad in ({"max_angle": 0}, {"max_angle": 91}, {"max_angle": 30, "rounds": 0}, {"max_angle": 30, "rounds": 65}):
        with pytest.raises(ValueError):
            flip.flip_edges(v, f, **bad)


def test_the_entry_points_refuse_bad_arguments_without_a_launch():
    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    t = torch.zeros((64,), dtype=torch.float64, device="cuda")
    o = torch.zeros((64,), dtype=torch.float64, device="cuda")
    p, q = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr())
    E = _lib.ERR_INVALID_ARG
    cand = lambda vertices=p, n=4, m=1, emax=3, c2=0.75, key=q, opp=q: lib.d3d_mesh_flip_candidates(vertices, n, p, m, p, p, p, p, p, p, emax, c2, key,
                                                                                                   opp, None)
    assert cand(emax=0) == 0 and cand(n=0, m=0, emax=0) == 0   # nothing to launch
    assert cand(vertices=None) == E and cand(key=None) == E and cand(opp=None) == E
    assert b"null pointer" in lib.d3d_last_error()
    assert cand(n=1 << 31) == E and cand(n=-1) == E and cand(m=(1 << 31) // 6 + 1) == E and cand(m=-1) == E
    assert cand(emax=1 << 31) == E and cand(emax=-1) == E
    for c2 in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert cand(c2=c2) == E
    assert b"cos2_max_angle" in lib.d3d_last_error()
    claim = lambda n=4, edges=p, emax=3, claim=q, n_win=q: lib.d3d_mesh_flip_claim(n, edges, p, p, p, emax, claim, n_win, None)
    assert claim(edges=None) == E and claim(claim=None) == E and claim(n_win=None) == E and claim(n=-1) == E and claim(n=1 << 31) == E
    assert claim(emax=-1) == E and claim(emax=1 << 31) == E
    apply_ = lambda faces=p, m=1, emax=3, out=q, win=q, n_win=q: lib.d3d_mesh_flip_apply(faces, m, p, p, p, p, emax, p, out, win, n_win, None)
    assert apply_(faces=None) == E and apply_(out=None) == E and apply_(win=None) == E and apply_(n_win=None) == E
    assert apply_(m=-1) == E and apply_(m=(1 << 31) // 6 + 1) == E and apply_(emax=-1) == E and apply_(out=p) == E
    assert b"distinct" in lib.d3d_last_error()
    torch.cuda.synchronize()
    assert not t.any() and not o.any()


# ----------------------------------------------------------------------------------------
# the mesh stage
# ----------------------------------------------------------------------------------------
def _views(vs):
    from deep3d_aerial_amd import mesh

    return [mesh.MeshView(v["K"], v["E"], torch.from_numpy(np.ascontiguousarray(v["depth"], np.float32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(v.get("confidence", np.ones_like(v["depth"])), np.float32)).cuda()) for v in vs]


def _stage():
    """The mesh stage's scene (pipeline_scene's seven views of a tilted plane): (views, border, voxel, its mesh)."""
    import pipeline_scene as PS
    import texture_scene as TS
    from deep3d_aerial_amd import mesh

    scene = PS.SceneViews()
    border, voxel = TS.scene_border(scene)
    mv = _views(scene.views)
    v, f = mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel), None, 2, 0.2, None)
    return mv, border, voxel, v, f


def test_build_and_write_flips_between_the_collapse_and_the_subdivision(tmp_path, monkeypatch):
    import mesh_scene as MS
    from deep3d_aerial_amd import collapse, flip, mesh, subdivide

    mv, border, voxel, want_v, want_f = _stage()
    called = []
    real = flip.flip_edges
    monkeypatch.setattr(flip, "flip_edges", lambda *a, **k: called.append(1) or real(*a, **k))
    settings = MS.pipeline_settings(str(tmp_path / "off.ply"), border, voxel)
    # without the key: the same PLY bytes as the mesh stage's own mesh, and no timing
    tm = {}
    v, f = mesh.build_and_write(mv, settings, timings=tm)
    mesh.write_ply(str(tmp_path / "want.ply"), want_v, want_f)
    assert not called and "mesh_flip_s" not in tm and (tmp_path / "off.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    # with it: the same mesh, flipped
    v1, f1 = mesh.build_and_write(mv, dict(settings, path=str(tmp_path / "on.ply"), flip={"max_angle": 30.0}), timings=tm)
    info = {}
    fv, ff = real(want_v, want_f, 30.0, info=info)
    print("mesh stage: %d faces; %s" % (want_f.shape[0], flip.summary_line(info)))
    assert called and tm["mesh_flip_s"] > 0 and info["flips"] > 0 and "mesh_collapse_s" not in tm
    assert _same(v1, want_v.cpu().numpy()) and _same(f1, ff.cpu().numpy()) and not torch.equal(ff, want_f)
    V, F = mesh.read_ply(str(tmp_path / "on.ply"))
    assert _same(fv, V) and _same(ff, F)
    # collapse, flip and subdivision together: the composition of the three, in that order, and a valid file
    both = dict(settings, path=str(tmp_path / "all.ply"), collapse={"min_edge": 1.0, "rounds": 4}, flip={"max_angle": 30.0, "rounds": 8},
                subdivide={"max_edge": 2.0, "rounds": 1})
    tm = {}
    got_v, got_f = mesh.build_and_write(mv, both, timings=tm)
    cv, cf = collapse.collapse(want_v, want_f, mv, 1.0, max_edge=2.0, rounds=4)
    fi = {}
    xv, xf = real(cv, cf, 30.0, rounds=8, info=fi)
    sv, sf = subdivide.subdivide(xv, xf, mv, 2.0, rounds=1)
    assert fi["flips"] > 0 and tm["mesh_collapse_s"] > 0 and tm["mesh_flip_s"] > 0 and tm["mesh_subdivide_s"] > 0
    assert _same(got_v, sv.cpu().numpy()) and _same(got_f, sf.cpu().numpy())
    V, F = mesh.read_ply(str(tmp_path / "all.ply"))
    assert _same(got_v, V) and _same(got_f, F) and F.min() >= 0 and F.max() < len(V)
    assert (F[:, 0] != F[:, 1]).all() and (F[:, 1] != F[:, 2]).all() and (F[:, 2] != F[:, 0]).all()
    with pytest.raises(ValueError, match="max_angle"):
        mesh.build_and_write(mv, dict(settings, flip={"max_angle": 0}))


def test_the_mesh_tool_with_clean_and_the_standalone_tool_write_the_same_bytes(tmp_path, capsys):
    from deep3d_aerial_amd import flip, mesh

    s = T.scene()
    src = str(tmp_path / "in.ply")
    mesh.write_ply(src, s["V"], s["F"])
    assert mesh.main(["--clean", src, "--out", str(tmp_path / "tool.ply"), "--flip", str(FS.MAX_ANGLE)]) == str(tmp_path / "tool.ply")
    assert "mesh flip: round 1:" in capsys.readouterr().out
    assert flip.main(["--mesh", src, "--out", str(tmp_path / "cli.ply"), "--max_angle", str(FS.MAX_ANGLE)]) == str(tmp_path / "cli.ply")
    assert "flipped mesh" in capsys.readouterr().out
    assert (tmp_path / "tool.ply").read_bytes() == (tmp_path / "cli.ply").read_bytes() != (tmp_path / "in.ply").read_bytes()
    V, F = mesh.read_ply(str(tmp_path / "cli.ply"))
    assert _same(V, s["V"]) and _same(F, s["out_f"])
    # the rounds flag reaches the stage, and after the decimation the flip still runs
    mesh.main(["--clean", src, "--out", str(tmp_path / "three.ply"), "--flip", str(FS.MAX_ANGLE), "--flip_rounds", "3"])
    assert _same(mesh.read_ply(str(tmp_path / "three.ply"))[1], s["detail"][2]["faces"])
    assert "reached the round limit" in capsys.readouterr().out
