"""The flip of the mesh edges whose flip removes a cap triangle: the numpy restatement of
tests/mesh_flip_scene.py, written from the rule's text (deep3d_aerial_amd/flip.py), checked on that file's scene: every crafted
piece ends as stated, refused by the test named for it and passed by the others; the invariants hold in every round; the chain
comes to rest; the face order and the rotation of the corners do not matter; settings, command-line errors, header and binding; and
the bench tool's torch comparator against the restatement.  tests/test_mesh_flip_gpu.py holds the kernels and the driver to this
file bit for bit."""
import os
import re
import sys

import numpy as np
import pytest

import mesh_flip_scene as FS
import test_mesh_subdivide as S

ALL = list(FS.TESTS)
_SCENE = {}


def scene():
    """The scene and its chain, computed once: V, F, cases, detail (per round), out_f, info."""
    if not _SCENE:
        V, F, cases = FS.build()
        detail = []
        out_v, out_f, info = FS.flip_numpy(V, F, detail=detail)
        _SCENE.update(V=V, F=F, cases=cases, detail=detail, out_v=out_v, out_f=out_f, info=info)
    return _SCENE


def _eid(d):
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(d["edges"])}
    return lambda a, b: index[(min(a, b), max(a, b))]


def face_set(F):
    return set(tuple(f) for f in S.canonical(F).tolist())


def _canon(*f):
    k = f.index(min(f))
    return (f[k], f[(k + 1) % 3], f[(k + 2) % 3])


def directed(F):
    """{directed edge: number of faces that hold it}"""
    use = {}
    for f in np.asarray(F).tolist():
        for i in range(3):
            k = (f[i], f[(i + 1) % 3])
            use[k] = use.get(k, 0) + 1
    return use


def edge_classes(F):
    """(boundary, twice_one_way, other): the undirected edges with one face; with two faces that do not hold it in opposite
    directions; with more than two faces."""
    dr = directed(F)
    boundary, one_way, other = set(), set(), set()
    for (a, b), k in S.edge_use(F).items():
        if k == 1:
            boundary.add((a, b))
        elif k > 2:
            other.add((a, b))
        elif dr.get((a, b), 0) != 1 or dr.get((b, a), 0) != 1:
            one_way.add((a, b))
    return boundary, one_way, other


# ----------------------------------------------------------------------------------------
# the restatement on the scene
# ----------------------------------------------------------------------------------------
def test_the_seed_meets_the_conditions_it_was_chosen_for():
    s = scene()
    info, d = s["info"], s["detail"][0]
    assert len(d["edges"]) > 4600 and len(d["edges"]) % 256 != 0
    assert info["candidates"][0] > 512 and 0 < info["winners"][0] < info["candidates"][0]
    # the chain ends with a round of no candidates before round 16: the fixed point, not the cap
    assert 2 < info["rounds"] < FS.ROUNDS and info["candidates"][-1] == 0 and info["winners"][-1] == 0 and not info["hit_max_rounds"]
    assert all(w > 0 for w in info["winners"][:-1]) and info["flips"] == sum(info["winners"]) > 600
    assert (s["detail"][-1]["key"] == -1).all() and np.array_equal(s["detail"][-1]["faces"], s["out_f"])
    # capped, the loop reports it
    v3, f3, i3 = FS.flip_numpy(s["V"], s["F"], rounds=3)
    assert i3["hit_max_rounds"] and i3["rounds"] == 3 and np.array_equal(f3, s["detail"][2]["faces"])


def test_every_crafted_piece_is_refused_by_the_test_named_for_it_and_passed_by_the_others():
    s = scene()
    F, c, d = s["F"], s["cases"], s["detail"][0]
    key, opp, win, passed = d["key"], d["opp"], d["win"], d["passed"]
    eid = _eid(d)
    got = lambda p: [k for k in ALL if passed[k][eid(p["a"], p["b"])]]
    without = lambda name: [k for k in ALL if k != name]
    valid = np.logical_and.reduce([passed[k] for k in ALL])
    assert ((key >= 0) == valid).all() and not opp[key < 0].any()
    # the two caps flip, the one without area too
    for name in ("cap", "zero"):
        p = c[name]
        e = eid(p["a"], p["b"])
        assert got(p) == ALL and win[e] and opp[e].tolist()[:2] == [p["c"], p["d"]]
        assert F[opp[e, 2]].tolist() == [p["a"], p["b"], p["c"]] and F[opp[e, 3]].tolist() == [p["b"], p["a"], p["d"]]
    X = s["V"].astype(np.float64).tolist()
    z = c["zero"]
    assert FS.quality(X, z["a"], z["b"], z["c"]) == 0.0 and key[eid(z["a"], z["b"])] >> 32 == 0 and key[eid(z["a"], z["b"])] == key[key >= 0].min()
    # no strict gain: the square keeps its diagonal
    r = c["regular"]
    assert got(r) == without("gain")
    assert FS.quality(X, r["a"], r["b"], r["c"]) == FS.quality(X, r["a"], r["d"], r["c"]) == 0.0625
    # rule 3: one face, three faces, two faces that hold the edge the same way
    t = c["boundary"]
    assert not any(passed["pair"][eid(t[i], t[j])] for i in range(3) for j in range(i + 1, 3))
    use = S.edge_use(F)
    for name, faces in (("three", 3), ("inconsistent", 2)):
        p = c[name]
        assert got(p) == [] and use[(p["a"], p["b"])] == faces
    assert directed(F)[(c["inconsistent"]["a"], c["inconsistent"]["b"])] == 2
    # rules 4 and 5, each alone
    assert got(c["exists"]) == without("new_edge") and c["exists"]["d"] in d["nbr"][d["offset"][c["exists"]["c"]]:d["offset"][c["exists"]["c"] + 1]]
    g = c["degree"]
    assert got(g) == without("degree") and d["offset"][g["a"] + 1] - d["offset"][g["a"]] == 3 < d["offset"][g["b"] + 1] - d["offset"][g["b"]]
    assert got(c["roof"]) == without("guard") and got(c["concave"]) == without("turn")
    # with a guard of 60 degrees the roof's 45 pass and it flips; the guard's own ends
    wide = FS.flip_round_numpy(s["V"], F, 60.0)
    assert wide["win"][eid(c["roof"]["a"], c["roof"]["b"])] and FS.cos2(90.0) < 1e-30 and 0.99 < FS.cos2(1.0) < 1.0
    # the two caps that share a vertex: both candidates, the worse one wins the vertex
    p1, p2 = c["shared"]
    e1, e2 = eid(p1["a"], p1["b"]), eid(p2["a"], p2["b"])
    assert p1["b"] == p2["a"] and got(p1) == got(p2) == ALL and key[e1] < key[e2] and win[e1] and not win[e2]
    assert d["claim"][p1["b"]] == key[e1] and d["claim"][p2["b"]] == key[e2]
    d2 = s["detail"][1]
    assert d2["win"][_eid(d2)(p2["a"], p2["b"])] and (p1["a"], p1["b"]) not in S.edge_use(d2["faces"])
    # the fan: the centre is the smaller end of 40 spokes that all reach the last test, and none gains
    centre, rim, ring = c["fan"]
    spokes = [eid(centre, x) for x in rim]
    assert d["face_offset"][centre + 1] - d["face_offset"][centre] == FS.FAN and all(d["edges"][k, 0] == centre for k in spokes)
    assert all([k for k in ALL if passed[k][e]] == without("gain") for e in spokes)
    assert c["unreferenced"] not in set(F.ravel().tolist())
    # the grid: the collisions are there, and winners share no vertex
    w = np.nonzero(win)[0]
    held = np.concatenate([d["edges"][w].ravel(), opp[w, :2].ravel()])
    assert len(set(held.tolist())) == 4 * len(w) and d["winners"] == len(w) < d["candidates"]


def test_every_piece_ends_as_stated():
    s = scene()
    F, c = s["F"], s["cases"]
    before, after = face_set(F), face_set(s["out_f"])
    flipped = [c["cap"], c["zero"]] + list(c["shared"])
    for p in flipped:
        a, b, cc, dd = p["a"], p["b"], p["c"], p["d"]
        assert {_canon(a, b, cc), _canon(b, a, dd)} <= before and not {_canon(a, b, cc), _canon(b, a, dd)} & after
        assert {_canon(a, dd, cc), _canon(b, cc, dd)} <= after
    for name in ("regular", "three", "inconsistent", "exists", "degree", "roof", "concave"):
        members = set(c[name].values())
        piece = set(f for f in before if set(f) <= members)
        assert len(piece) >= 2 and piece <= after, name
    members = set([c["fan"][0]] + c["fan"][1] + c["fan"][2]) | set(c["boundary"])
    assert set(f for f in before if set(f) <= members) == set(f for f in after if set(f) <= members)
    # every flip happened where it was written: a face slot changes only by a flip
    changed = np.nonzero((F != s["out_f"]).any(1))[0]
    assert len(changed) <= 2 * s["info"]["flips"] and len(changed) > 600


def test_the_invariants_hold_in_every_round():
    s = scene()
    V, F = s["V"], s["F"]
    classes = edge_classes(F)
    c = s["cases"]
    assert classes[1] == {(c["inconsistent"]["a"], c["inconsistent"]["b"])} and classes[2] == {(c["three"]["a"], c["three"]["b"])}
    q = FS.qualities(V, F)
    P = V.astype(np.float64)
    for d in s["detail"]:
        G = d["faces"]
        assert d["vertices"].tobytes() == V.tobytes() and G.shape == F.shape and G.dtype == np.int32
        if d["winners"] == 0:
            assert np.array_equal(G, F)
            continue
        # the boundary, the non-manifold edges and the orientation of every interior edge
        assert edge_classes(G) == classes
        assert (G[:, 0] != G[:, 1]).all() and (G[:, 1] != G[:, 2]).all() and (G[:, 2] != G[:, 0]).all()
        # no face turned over against the normal of the pair it came from
        w = np.nonzero(d["win"])[0]
        fab, fba = d["opp"][w, 2], d["opp"][w, 3]
        nrm = lambda T: np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
        pair = nrm(F[fab]) + nrm(F[fba])
        assert ((nrm(G[fab]) * pair).sum(1) > 0).all() and ((nrm(G[fba]) * pair).sum(1) > 0).all()
        # the winners' slots are the only ones written
        same = np.ones(len(F), bool)
        same[fab] = same[fba] = False
        assert np.array_equal(G[same], F[same]) and len(set(fab.tolist() + fba.tolist())) == 2 * len(w)
        # the ascending qualities grow lexicographically
        q2 = FS.qualities(V, G)
        assert q2 > q
        q, F = q2, G
    assert np.array_equal(F, s["out_f"])


def test_permuting_the_faces_and_rotating_their_corners_give_the_same_face_set():
    s = scene()
    want = S.canonical(s["out_f"])
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(s["F"]))
    v2, f2, info2 = FS.flip_numpy(s["V"], s["F"][perm])
    assert np.array_equal(S.canonical(f2), want) and info2 == s["info"]
    turn = rng.integers(0, 3, len(s["F"]))
    rolled = np.stack([s["F"][np.arange(len(turn)), (turn + i) % 3] for i in range(3)], 1)
    assert (turn > 0).sum() > 1000 and np.array_equal(S.canonical(rolled), S.canonical(s["F"]))
    v3, f3, info3 = FS.flip_numpy(s["V"], rolled[perm])
    assert np.array_equal(S.canonical(f3), want) and info3 == s["info"]
    # the keys of round 1 do not depend on either
    r = FS.flip_round_numpy(s["V"], rolled)
    assert np.array_equal(r["key"], s["detail"][0]["key"]) and np.array_equal(r["opp"][:, :2], s["detail"][0]["opp"][:, :2])


# ----------------------------------------------------------------------------------------
# settings, command line, header
# ----------------------------------------------------------------------------------------
def test_settings_are_checked():
    from deep3d_aerial_amd import flip, mesh

    assert flip.check_flip_settings({"max_angle": 30}) == {"max_angle": 30.0, "rounds": 16}
    assert flip.check_flip_settings({"max_angle": 90, "rounds": 64}) == {"max_angle": 90.0, "rounds": 64}
    assert flip.check_flip_settings({"max_angle": "12.5", "rounds": None}) == {"max_angle": 12.5, "rounds": 16}
    for bad in ({}, {"max_angle": None}, {"max_angle": 0}, {"max_angle": -5}, {"max_angle": 91}, {"max_angle": float("nan")},
                {"max_angle": float("inf")}, {"max_angle": "x"}, {"rounds": 4}, {"max_angle": 30, "rounds": 0}, {"max_angle": 30, "rounds": 65},
                {"max_angle": 30, "rounds": 2.5}, {"max_angle": 30, "rounds": "x"}, {"max_angle": 30, "reach": 1},
                {"max_angle": 30, "views_per_batch": 2}):
        with pytest.raises(ValueError):
            flip.check_flip_settings(bad)
    assert flip.cos2(30.0) == FS.cos2(30.0) and abs(flip.cos2(30.0) - 0.75) < 1e-15 and 0 <= flip.cos2(90.0) < 1e-30
    # the mesh settings carry it under "flip"
    assert mesh.flip_settings({"views_per_batch": 3}) is None
    assert mesh.flip_settings({"flip": {"max_angle": 20, "rounds": 2}}) == {"max_angle": 20.0, "rounds": 2}
    for bad in ({"max_angle": 0}, {"rounds": 2}, {"max_angle": 91}, {"max_angle": 30, "depth_tolerance": 0.01}):
        with pytest.raises(ValueError):
            mesh.flip_settings({"flip": bad})


def test_the_flags_parse_in_mesh_flip_and_predict(capsys):
    import argparse

    from deep3d_aerial_amd import flip, mesh, predict

    ap = argparse.ArgumentParser()
    mesh.add_arguments(ap, prefix="mesh_")
    base = ["--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.1"]
    a = ap.parse_args(base)
    assert "flip" not in mesh.settings_from_args(a, "m.ply", "mesh_")   # the key is carried only when the flag is given
    a = ap.parse_args(base + ["--mesh_flip", "30", "--mesh_flip_rounds", "3"])
    s = mesh.settings_from_args(a, "m.ply", "mesh_")
    assert s["flip"] == {"max_angle": 30.0, "rounds": 3} and "collapse" not in s and "subdivide" not in s
    mesh.check_args(ap, a, "mesh_")
    for bad in (["--mesh_flip", "0"], ["--mesh_flip", "91"], ["--mesh_flip", "30", "--mesh_flip_rounds", "65"]):
        with pytest.raises(SystemExit):
            mesh.check_args(ap, ap.parse_args(base + bad), "mesh_")
        assert "flip" in capsys.readouterr().err
    # the mesh tool takes the flip with --clean too: it needs no views
    for bad in (["--flip", "0"], ["--flip", "30", "--flip_rounds", "0"]):
        with pytest.raises(SystemExit):
            mesh.main(["--clean", "in.ply", "--out", "out.ply"] + bad)
        assert "flip" in capsys.readouterr().err
    # the stand-alone tool
    tool = ["--mesh", "m.ply", "--out", "o.ply"]
    for bad in (tool, tool + ["--max_angle", "0"], tool + ["--max_angle", "91"], tool + ["--max_angle", "30", "--rounds", "0"],
                tool + ["--max_angle", "30", "--rounds", "65"], tool[:2] + ["--out", "o.obj", "--max_angle", "30"], tool + ["--max_angle"]):
        with pytest.raises(SystemExit):
            flip.main(bad)
    capsys.readouterr()
    # predict takes the flags through mesh.add_arguments, carries the key only with the flag, and reports the time
    base = ["--model", "casmvsnet", "--loadckpt", "x.ckpt", "--data_folder", "d", "--output_folder", "o", "--fuse"]
    on = base + ["--mesh", "m.ply", "--mesh_border", "0,1,0,1,0,1", "--mesh_voxel", "0.1"]
    assert "flip" not in predict._mesh_settings(predict.parse_args(on))
    s = predict._mesh_settings(predict.parse_args(on + ["--mesh_flip", "25", "--mesh_flip_rounds", "8"]))
    assert mesh.flip_settings(s) == {"max_angle": 25.0, "rounds": 8}
    for bad, what in ((on + ["--mesh_flip", "-1"], "max_angle"), (on + ["--mesh_flip", "30", "--mesh_flip_rounds", "99"], "rounds"),
                      (base + ["--mesh_flip", "30"], "--mesh_flip needs --mesh")):
        with pytest.raises(SystemExit):
            predict.parse_args(bad)
        assert what in capsys.readouterr().err
    assert "mesh_flip_s" in open(predict.__file__).read()


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib, flip

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    for name in ("d3d_mesh_flip_candidates", "d3d_mesh_flip_claim", "d3d_mesh_flip_apply"):
        assert re.search(r"\bint %s\(" % name, text) and name in _lib.SIGNATURES
    assert "mesh_flip.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "does not claim to match" in flip.__doc__ and "a setting, not a measurement" in flip.__doc__
    source = open(os.path.join(_lib.CSRC, "mesh_flip.hip")).read()
    assert "does not claim to match" in source and set(re.findall(r"atomic[A-Z]\w*", source)) == {"atomicMin", "atomicAdd"}
    assert "double*)" not in source.split("atomicAdd(")[1][:40]   # the one atomicAdd is the integer counter


def test_the_bench_tools_torch_comparator_equals_the_restatement():
    """tools/mesh_flip_bench.py's fp64 torch candidates, on CPU tensors, against the restatement's key and opp on two rounds of
    the scene."""
    import torch

    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import mesh_flip_bench as B

    s = scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for k in (0, 3):
        d = s["detail"][k]
        f = s["F"] if k == 0 else s["detail"][k - 1]["faces"]
        topo = {"offset": t(d["offset"]), "nbr": t(d["nbr"]), "face_offset": t(d["face_offset"]), "face_index": t(d["face_index"])}
        key, opp = B.torch_candidates(t(s["V"]), t(f), topo, t(d["edges"]), FS.MAX_ANGLE)
        assert np.array_equal(key.numpy(), d["key"]) and np.array_equal(opp.numpy(), d["opp"]) and (d["key"] >= 0).sum() > 200
    # the tool's mesh is the scene's kind of grid, and its byte counts are the docstring's
    v, f = B.grid_mesh(9, "cpu")
    assert v.shape == (81, 3) and f.shape == (128, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
    assert len(S.edge_use(f.numpy())) == 8 * 9 * 2 + 64 and edge_classes(f.numpy())[1:] == (set(), set())
    assert B.pass_bytes(10, 20, 30, 4) == {"candidates": 1200 + 240 + 480, "claim": 80 + 240 + 224, "apply": 480 + 270 + 224}
