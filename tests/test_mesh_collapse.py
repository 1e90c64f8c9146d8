"""The collapse of the mesh edges the images cannot resolve restated in numpy from the rule's text
(deep3d_aerial_amd/collapse.py), and that restatement checked on the scene of tests/mesh_collapse_scene.py: every crafted case ends as
intended, the loop comes to rest, every round removes vertices, the boundary keeps its bits, the face order does not matter;
settings, command-line errors, header and binding.  The measure is tests/test_mesh_subdivide.py's restatement and the claim, apply
and faces passes are tests/test_mesh_decimate.py's, imported rather than copied.  tests/test_mesh_collapse_gpu.py holds the kernel
and the driver to this file bit for bit."""
import os
import re

import numpy as np
import pytest

import mesh_collapse_scene as CS
import test_mesh_decimate as D
import test_mesh_subdivide as S

HASH = 2654435761
TESTS = ("short", "free", "link", "degree", "guard", "flips")
_SCENE = {}


# ----------------------------------------------------------------------------------------
# the rule in numpy (Python floats: fp64, one operation at a time, nothing contracted)
# ----------------------------------------------------------------------------------------
def _d2(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def _normal(p0, p1, p2):
    ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    vx, vy, vz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return (uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx)


def _flips(X, F, foff, finc, v, other, t):
    """Test 3 over the faces of v that do not hold `other`, with v at t."""
    for f in finc[foff[v]:foff[v + 1]].tolist():
        tri = F[f]
        if other in tri:
            continue
        p = [X[i] for i in tri]
        n0 = _normal(*p)
        p[tri.index(v)] = t
        n1 = _normal(*p)
        if not (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0:
            return True
    return False


def candidates_numpy(V, F, offset, nbr, fixed, foff, finc, E, measure, min_edge, max_edge, passed=None):
    """Rule 4: (target [E,3] fp32, key [E] int64).  passed (a dict) gets per test name a bool [E] array: the edge got to the test
    and passed it."""
    V = np.asarray(V, np.float32)
    X = V.astype(np.float64).tolist()
    F = np.asarray(F).tolist()
    rows = [nbr[offset[v]:offset[v + 1]].tolist() for v in range(len(V))]
    min2, max2 = float(min_edge) * float(min_edge), float(max_edge) * float(max_edge)
    target = np.zeros((len(E), 3), np.float32)
    key = np.full(len(E), -1, np.int64)
    ok = {k: np.zeros(len(E), bool) for k in TESTS}
    for e, (a, b) in enumerate(np.asarray(E).tolist()):
        m = float(measure[e])
        if not (0.0 < m < min2):
            continue
        ok["short"][e] = True
        fa, fb = bool(fixed[a]), bool(fixed[b])
        if fa and fb:
            continue
        ok["free"][e] = True
        if len(set(rows[a]) & set(rows[b])) != 2:
            continue
        ok["link"][e] = True
        if len(rows[a]) + len(rows[b]) - 4 < 3:
            continue
        ok["degree"][e] = True
        if fa or fb:
            t32 = V[a] if fa else V[b]
        else:
            t32 = np.array([(X[a][i] + X[b][i]) * 0.5 for i in range(3)], np.float64).astype(np.float32)
        t = t32.astype(np.float64).tolist()
        with np.errstate(all="ignore"):
            s = np.float64(m) / np.float64(_d2(X[b], X[a]))
            guard = all(bool(np.float64(_d2(t, X[w])) * s <= max2) for w in rows[a] + rows[b] if w != a and w != b)
        if not guard:
            continue
        ok["guard"][e] = True
        if _flips(X, F, foff, finc, a, b, t) or _flips(X, F, foff, finc, b, a, t):
            continue
        ok["flips"][e] = True
        target[e] = t32
        key[e] = (int(np.float32(m).view(np.uint32)) << 32) | ((e * HASH) & 0xFFFFFFFF)
    if passed is not None:
        passed.update(ok)
    return target, key


def collapse_round_numpy(V, F, views, min_edge=CS.MIN_EDGE, max_edge=CS.MAX_EDGE, tol=CS.TOLERANCE):
    """One round (rules 2-5): test_mesh_decimate's round with this file's candidates in the place of the quadric ones and every
    valid key eligible (a target so far below the face count that K is at least the number of edges).  The dict of every pass:
    edges, measure, passed, target, key, claim, win, remap, winners, short, valid, and the mesh after it (vertices, faces)."""
    V, F = np.asarray(V, np.float32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    extra = {}

    def candidates(v, f, offset, nbr, fixed, foff, finc, Q, edges):
        measure = S.measure_numpy(v, edges, views, tol)
        passed = {}
        target, key = candidates_numpy(v, f, offset, nbr, fixed, foff, finc, edges, measure, min_edge, max_edge, passed)
        extra.update(measure=measure, passed=passed)
        return target, np.zeros(len(edges), np.float32), key

    theirs = D.candidates_numpy
    D.candidates_numpy = candidates
    try:
        out = D.decimate_round_numpy(V, F, -6 * len(F) - 6)
    finally:
        D.candidates_numpy = theirs
    out.update(extra)
    E, win = out["edges"], out["win"] != 0
    keep_b = (out["fixed"][E[:, 1]] != 0) & (out["fixed"][E[:, 0]] == 0)
    remap = np.arange(len(V), dtype=np.int32)
    remap[np.where(keep_b, E[:, 0], E[:, 1])[win]] = np.where(keep_b, E[:, 1], E[:, 0])[win]
    m = out["measure"]
    out.update(remap=remap, short=int(((m > 0) & (m < float(min_edge) * float(min_edge))).sum()), valid=int((out["key"] >= 0).sum()))
    return out


def collapse_numpy(V, F, views, min_edge=CS.MIN_EDGE, max_edge=CS.MAX_EDGE, rounds=CS.ROUNDS, tol=CS.TOLERANCE, detail=None):
    """Rule 6: (vertices, faces, info) as collapse.collapse; detail (a list) gets every round's dict."""
    V, F = np.asarray(V, np.float32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    info = {"edges": [], "short": [], "valid": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces_in": len(F)}
    for k in range(rounds if len(V) and len(F) else 0):
        r = collapse_round_numpy(V, F, views, min_edge, max_edge, tol)
        if detail is not None:
            detail.append(r)
        info["rounds"] += 1
        info["edges"].append(len(r["edges"]))
        for name in ("short", "valid", "winners"):
            info[name].append(r[name])
        if r["winners"] == 0:
            break
        V, F = r["vertices"], r["faces"]
        info["hit_max_rounds"] = k + 1 == rounds
    info.update(faces_out=len(F), vertices_out=len(V))
    return V, F, info


def scene():
    """The scene and its chain, computed once: V, F, cases, views, detail (per round), out_v, out_f, info."""
    if not _SCENE:
        views = CS.numpy_views()
        V, F, cases = CS.build(views)
        detail = []
        out_v, out_f, info = collapse_numpy(V, F, views, detail=detail)
        _SCENE.update(V=V, F=F, cases=cases, views=views, detail=detail, out_v=out_v, out_f=out_f, info=info)
    return _SCENE


# ----------------------------------------------------------------------------------------
# helpers of the checks
# ----------------------------------------------------------------------------------------
def _eid(d):
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(d["edges"])}
    return lambda a, b: index[(min(a, b), max(a, b))]


def _pos(V, i):
    return np.asarray(V, np.float32)[int(i)].tobytes()


def face_positions(V, F):
    """Every face as the positions of its corners (bytes), the smallest first with the winding kept: a set."""
    out = set()
    for f in np.asarray(F).tolist():
        p = [_pos(V, i) for i in f]
        k = p.index(min(p))
        out.add((p[k], p[(k + 1) % 3], p[(k + 2) % 3]))
    return out


def piece_faces(F, members):
    members = set(int(x) for x in members)
    return np.array([f for f in np.asarray(F).tolist() if f[0] in members], np.int32).reshape(-1, 3)


def guard_ratios(s, d, a, b, others):
    """(|t - x_w|^2 s) / max_edge^2 of test 4 for the both-free edge a-b and the neighbours `others`."""
    X = s["V"].astype(np.float64)
    t = ((X[a] + X[b]) * 0.5).astype(np.float32).astype(np.float64)
    scale = d["measure"][_eid(d)(a, b)] / _d2(X[b].tolist(), X[a].tolist())
    return np.array([_d2(t.tolist(), X[w].tolist()) * scale / CS.MAX_EDGE ** 2 for w in others])


# ----------------------------------------------------------------------------------------
# the restatement on the scene
# ----------------------------------------------------------------------------------------
def test_the_scene_holds_every_crafted_case_in_its_first_round():
    s = scene()
    V, F, c, d = s["V"], s["F"], s["cases"], s["detail"][0]
    E, m, key, win, passed, fixed, target = d["edges"], d["measure"], d["key"], d["win"], d["passed"], d["fixed"], d["target"]
    eid = _eid(d)
    got = lambda a, b: [k for k in TESTS if passed[k][eid(a, b)]]
    assert len(E) > 2 * 256 and (key[~passed["flips"]] == -1).all() and (key[passed["flips"]] >= 0).all()
    assert not target[key < 0].any()
    # the grid: hundreds of short interior edges, a fixed boundary with short edges that stay, interior edges that collapse onto it
    g = c["grid"]
    inner, members = set(g[1:-1, 1:-1].ravel().tolist()), set(g.ravel().tolist())
    ge = [k for k, (a, b) in enumerate(E.tolist()) if a in members and b in members]
    assert passed["short"][ge].all() and len(ge) > 350
    assert all(bool(fixed[v]) != (v in inner) for v in members)
    bb = [k for k in ge if E[k, 0] not in inner and E[k, 1] not in inner]
    assert len(bb) == 4 * (CS.GRID_N - 1) + 2 and not passed["free"][bb].any() and (key[bb] == -1).all()
    onto = [k for k in ge if (E[k, 0] in inner) != (E[k, 1] in inner) and key[k] >= 0]
    assert len(onto) > 40
    for k in onto:
        keep = E[k, 0] if E[k, 0] not in inner else E[k, 1]
        assert target[k].tobytes() == _pos(V, keep)
    both = [k for k in ge if E[k, 0] in inner and E[k, 1] in inner and key[k] >= 0]
    X = V.astype(np.float64)
    assert len(both) > 200 and all(target[k].tobytes() == ((X[E[k, 0]] + X[E[k, 1]]) * 0.5).astype(np.float32).tobytes() for k in both)
    # the fan: a row of 40, every spoke a valid candidate, one winner
    centre, rim = c["fan"]
    spokes = [eid(centre, r) for r in rim]
    assert d["offset"][centre + 1] - d["offset"][centre] == CS.FAN > 32 and not fixed[centre] and fixed[rim].all()
    assert (key[spokes] >= 0).all() and win[spokes].sum() == 1 and key[spokes].min() == key[spokes][win[spokes] != 0][0]
    assert not any(passed["free"][eid(rim[i], rim[(i + 1) % CS.FAN])] for i in range(CS.FAN))
    # test 3 alone refuses a-b of the flip piece; the shortest spoke of a is valid and wins
    f = c["flip"]
    assert got(f["a"], f["b"]) == ["short", "free", "link", "degree", "guard"] and key[eid(f["a"], f["b"])] == -1
    e1 = eid(f["a"], f["r1"])
    assert win[e1] and m[e1] == min(m[eid(f["a"], r)] for r in f["ring"])
    # test 1 refuses a-b of "three", and no other edge of the piece is short
    t3 = c["three"]
    assert got(t3["a"], t3["b"]) == ["short", "free"]
    assert len(set(d["nbr"][d["offset"][t3["a"]]:d["offset"][t3["a"] + 1]]) & set(d["nbr"][d["offset"][t3["b"]]:d["offset"][t3["b"] + 1]])) == 3
    assert [k for k, (a, b) in enumerate(E.tolist()) if a in t3["all"] and passed["short"][k]] == [eid(t3["a"], t3["b"])]
    # test 2 refuses every edge of the tetrahedron
    tet = c["tetra"]
    assert not fixed[list(tet)].any()
    assert all(got(tet[i], tet[j]) == ["short", "free", "link"] for i in range(4) for j in range(i + 1, 4))
    # test 4 refuses the far needle and passes the near one, neither within rounding of equality
    a, b, others = c["needle_far"]
    far = guard_ratios(s, d, a, b, others)
    assert got(a, b) == ["short", "free", "link", "degree"] and (far > 1.5).all() and not fixed[[a, b]].any()
    a, b, others = c["needle_near"]
    near = guard_ratios(s, d, a, b, others)
    assert got(a, b) == list(TESTS) and (near < 0.9).all() and (near > 0.5).all() and win[eid(a, b)]
    # the equal pair: one fp32 measure, so the keys differ in the hash alone; the fp64 measures differ; both win
    (a1, b1, _), (a2, b2, _), k = c["equal"]
    e1, e2 = eid(a1, b1), eid(a2, b2)
    assert m[e1] != m[e2] and np.float32(m[e1]).tobytes() == np.float32(m[e2]).tobytes()
    assert key[e1] >> 32 == key[e2] >> 32 and key[e1] != key[e2] and win[e1] and win[e2]
    per_view = [S.edge_l2_numpy(v, V, E[[e1, e2]]) for v in s["views"]]
    assert int(np.argmax([p[0] for p in per_view])) == k == int(np.argmax([p[1] for p in per_view]))
    # measure 0: hidden behind the plane or outside every image, so not short, however small and free
    for name in ("hidden", "outside"):
        centre, rim = c[name]
        assert not fixed[centre] and all(m[eid(centre, r)] == 0 and got(centre, r) == [] for r in rim)
        assert all(_d2(X[centre].tolist(), X[r].tolist()) < 1.1 for r in rim)
    inside = [S.seen_numpy(v, X[[c["hidden"][0]]], 1e9)[0][0] for v in s["views"]]   # the depth test switched off
    assert any(inside) and not any(S.seen_numpy(v, X[[c["outside"][0]]], 1e9)[0][0] for v in s["views"])
    assert c["unreferenced"] not in set(F.ravel().tolist())
    assert d["winners"] == 6 and d["short"] == int(passed["short"].sum()) and d["valid"] == int(passed["flips"].sum())


def test_every_case_ends_as_intended_and_the_loop_comes_to_rest():
    s = scene()
    V, F, c, info = s["V"], s["F"], s["cases"], s["info"]
    out_v, out_f = s["out_v"], s["out_f"]
    # the loop stops by itself: its last round has short edges left (the boundary's) and no valid candidate
    assert 2 < info["rounds"] < CS.ROUNDS and not info["hit_max_rounds"]
    assert info["winners"][-1] == 0 and info["valid"][-1] == 0 and info["short"][-1] > 0 and all(w > 0 for w in info["winners"][:-1])
    last = s["detail"][-1]
    assert np.array_equal(last["vertices"], out_v) and np.array_equal(last["faces"], out_f) and (last["key"] == -1).all()
    # every round removes as many vertices as it has winners (the first also the vertex no face uses) and two faces per winner
    n, m = len(V), len(F)
    for k, r in enumerate(s["detail"][:-1]):
        assert len(r["vertices"]) == n - r["winners"] - (1 if k == 0 else 0) < n and len(r["faces"]) == m - 2 * r["winners"]
        n, m = len(r["vertices"]), len(r["faces"])
    assert info["faces_out"] == len(out_f) == m and info["vertices_out"] == len(out_v) == n and info["faces_in"] == len(F)
    # capped, the loop reports it
    v3, f3, i3 = collapse_numpy(V, F, s["views"], rounds=3)
    assert i3["hit_max_rounds"] and i3["rounds"] == 3 and np.array_equal(f3, s["detail"][2]["faces"])
    # the pieces the rule refuses come back face for face
    after = face_positions(out_v, out_f)
    have = set(out_v[i].tobytes() for i in range(len(out_v)))
    for name, members in (("three", c["three"]["all"]), ("tetra", c["tetra"]), ("needle_far", c["needle_far"][:2]),
                          ("hidden", c["hidden"][:1]), ("outside", c["outside"][:1])):
        assert face_positions(V, piece_faces(F, members)) <= after, name
    # the near needles (the equal pair too) lose the edge: a and b are gone, the midpoint is there, four faces are left
    X = V.astype(np.float64)
    for a, b, others in (c["needle_near"], c["equal"][0][:3], c["equal"][1][:3]):
        mid = ((X[a] + X[b]) * 0.5).astype(np.float32).tobytes()
        assert mid in have and _pos(V, a) not in have and _pos(V, b) not in have
        ring = set(_pos(V, w) for w in others)
        assert sum(1 for f in after if mid in f and len(set(f) & ring) == 2) == 4
    # the fan's centre went onto a rim vertex: 38 faces over the 40 rim vertices; the flip piece's a went onto r1
    centre, rim = c["fan"]
    rim_pos = set(_pos(V, r) for r in rim)
    assert _pos(V, centre) not in have and rim_pos <= have and sum(1 for f in after if set(f) <= rim_pos) == CS.FAN - 2
    f = c["flip"]
    ring_pos = set(_pos(V, r) for r in f["ring"])
    assert _pos(V, f["a"]) not in have and ring_pos <= have and sum(1 for t in after if set(t) <= ring_pos) == 3
    # the grid keeps its boundary and loses most of its interior
    g = c["grid"]
    border = set(_pos(V, v) for v in g.ravel().tolist()) - set(_pos(V, v) for v in g[1:-1, 1:-1].ravel().tolist())
    assert len(border) == 4 * (CS.GRID_N - 1) and border <= have
    assert sum(1 for v in g[1:-1, 1:-1].ravel().tolist() if _pos(V, v) in have) < 10
    assert _pos(V, c["unreferenced"]) not in have
    # the boundary vertices come through with their bits, and nothing else becomes boundary
    fixed0 = D.C.adjacency_numpy(len(V), F)[2] != 0
    used0 = np.zeros(len(V), bool)
    used0[F.ravel()] = True
    fixed1 = D.C.adjacency_numpy(len(out_v), out_f)[2] != 0
    assert sorted(V[fixed0 & used0].view(np.uint32).tolist()) == sorted(out_v[fixed1].view(np.uint32).tolist())
    assert (D._areas(out_v, out_f) > 0).all() and len(np.unique(out_f)) == len(out_v)


def test_permuting_the_faces_gives_the_same_mesh():
    s = scene()
    perm = np.random.default_rng(5).permutation(len(s["F"]))
    v2, f2, info2 = collapse_numpy(s["V"], s["F"][perm], s["views"])
    assert np.array_equal(v2.view(np.uint32), s["out_v"].view(np.uint32))
    assert np.array_equal(S.canonical(f2), S.canonical(s["out_f"])) and info2 == s["info"]


def test_the_result_does_not_depend_on_the_view_order():
    s = scene()
    r = collapse_round_numpy(s["V"], s["F"], s["views"][::-1])
    d = s["detail"][0]
    assert np.array_equal(r["measure"], d["measure"]) and np.array_equal(r["key"], d["key"]) and np.array_equal(r["faces"], d["faces"])
    # fewer views see less: with the first view alone some edges are no longer measured, and nothing unseen is touched
    one = collapse_round_numpy(s["V"], s["F"], s["views"][:1])
    assert 0 < (one["measure"] > 0).sum() < (d["measure"] > 0).sum() and (one["key"][one["measure"] == 0] == -1).all()
    none = collapse_round_numpy(s["V"], s["F"], [])
    assert none["winners"] == 0 and none["short"] == 0 and len(none["faces"]) == len(s["F"])


# ----------------------------------------------------------------------------------------
# settings, command line, header
# ----------------------------------------------------------------------------------------
def test_settings_are_checked():
    from deep3d_aerial_amd import collapse, mesh

    s = collapse.check_collapse_settings({"min_edge": 1})
    assert s == {"min_edge": 1.0, "max_edge": 4.0, "rounds": 16, "depth_tolerance": 0.01, "views_per_batch": None}
    s = collapse.check_collapse_settings({"min_edge": 0.5, "max_edge": 1, "rounds": 64, "depth_tolerance": 0, "views_per_batch": 2})
    assert s == {"min_edge": 0.5, "max_edge": 1.0, "rounds": 64, "depth_tolerance": 0.0, "views_per_batch": 2}
    for bad in ({}, {"min_edge": None}, {"min_edge": 0}, {"min_edge": -1}, {"min_edge": float("nan")}, {"min_edge": float("inf")},
                {"min_edge": "x"}, {"min_edge": 1, "max_edge": 1.5}, {"min_edge": 1, "max_edge": float("inf")},
                {"min_edge": 1, "max_edge": float("nan")}, {"min_edge": 1, "max_edge": "x"},
                {"min_edge": 1, "rounds": 0}, {"min_edge": 1, "rounds": 65}, {"min_edge": 1, "rounds": 2.5},
                {"min_edge": 1, "depth_tolerance": -1}, {"min_edge": 1, "depth_tolerance": float("nan")},
                {"min_edge": 1, "views_per_batch": 0}, {"min_edge": 1, "reach": 1}):
        with pytest.raises(ValueError):
            collapse.check_collapse_settings(bad)
    # the mesh settings carry it under "collapse", with their own views_per_batch
    assert mesh.collapse_settings({"views_per_batch": 3}) is None
    got = mesh.collapse_settings({"views_per_batch": 3, "collapse": {"min_edge": 2, "max_edge": 5, "rounds": 2, "depth_tolerance": 0.02}})
    assert got == {"min_edge": 2.0, "max_edge": 5.0, "rounds": 2, "depth_tolerance": 0.02, "views_per_batch": 3}
    for bad in ({"min_edge": 0}, {"rounds": 2}, {"min_edge": 1, "views_per_batch": 2}, {"min_edge": 1, "max_edge": 1}):
        with pytest.raises(ValueError):
            mesh.collapse_settings({"collapse": bad})
    # without a max_edge of its own the collapse takes the subdivision's, and refuses one below 2 min_edge
    both = {"collapse": {"min_edge": 1.5}, "subdivide": {"max_edge": 3}}
    assert mesh.collapse_settings(both)["max_edge"] == 3.0 and mesh.collapse_settings({"collapse": {"min_edge": 1.5}})["max_edge"] == 6.0
    assert mesh.collapse_settings(dict(both, collapse={"min_edge": 1.5, "max_edge": 8}))["max_edge"] == 8.0
    with pytest.raises(ValueError, match="2 min_edge"):
        mesh.collapse_settings({"collapse": {"min_edge": 2}, "subdivide": {"max_edge": 3}})


def test_the_flags_parse_and_clean_has_no_views(capsys):
    import argparse

    from deep3d_aerial_amd import collapse, mesh, predict

    ap = argparse.ArgumentParser()
    mesh.add_arguments(ap, prefix="mesh_")
    base = ["--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.1"]
    a = ap.parse_args(base)
    assert "collapse" not in mesh.settings_from_args(a, "m.ply", "mesh_")   # the key is carried only when the flag is given
    a = ap.parse_args(base + ["--mesh_collapse", "1", "--mesh_collapse_rounds", "3"])
    s = mesh.settings_from_args(a, "m.ply", "mesh_")
    assert s["collapse"] == {"min_edge": 1.0, "max_edge": None, "rounds": 3, "depth_tolerance": collapse.DEFAULT_TOLERANCE}
    assert "subdivide" not in s and mesh.collapse_settings(s)["max_edge"] == 4.0
    mesh.check_args(ap, a, "mesh_")
    a = ap.parse_args(base + ["--mesh_collapse", "1", "--mesh_collapse_max_edge", "2.5", "--mesh_subdivide", "6"])
    s = mesh.settings_from_args(a, "m.ply", "mesh_")
    assert s["collapse"]["max_edge"] == 2.5 and mesh.collapse_settings(s)["max_edge"] == 2.5
    s = mesh.settings_from_args(ap.parse_args(base + ["--mesh_collapse", "1", "--mesh_subdivide", "6"]), "m.ply", "mesh_")
    assert mesh.collapse_settings(s)["max_edge"] == 6.0   # the subdivision's
    for bad in (["--mesh_collapse", "0"], ["--mesh_collapse", "1", "--mesh_collapse_rounds", "65"],
                ["--mesh_collapse", "1", "--mesh_collapse_max_edge", "1.5"], ["--mesh_collapse", "2", "--mesh_subdivide", "3"]):
        with pytest.raises(SystemExit):
            mesh.check_args(ap, ap.parse_args(base + bad), "mesh_")
    assert "collapse" in capsys.readouterr().err
    # the mesh tool: --clean has no views
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--out", "out.ply", "--collapse", "1"])
    assert "--collapse needs the views" in capsys.readouterr().err
    # the stand-alone tool
    tool = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in (tool, tool + ["--min_edge", "0"], tool + ["--min_edge", "1", "--max_edge", "1.5"], tool + ["--min_edge", "1", "--rounds", "0"],
                tool + ["--min_edge", "1", "--depth_tolerance", "-1"], tool[:4] + ["--out", "o.obj", "--min_edge", "1"],
                tool + ["--min_edge", "1", "--views_per_batch", "0"]):
        with pytest.raises(SystemExit):
            collapse.main(bad)
    capsys.readouterr()
    # predict takes the flags through mesh.add_arguments, carries the key only with the flag, and reports the time
    base = ["--model", "casmvsnet", "--loadckpt", "x.ckpt", "--data_folder", "d", "--output_folder", "o", "--fuse"]
    on = base + ["--mesh", "m.ply", "--mesh_border", "0,1,0,1,0,1", "--mesh_voxel", "0.1"]
    assert "collapse" not in predict._mesh_settings(predict.parse_args(on))
    s = predict._mesh_settings(predict.parse_args(on + ["--mesh_collapse", "0.75", "--mesh_collapse_max_edge", "2"]))
    assert mesh.collapse_settings(s) == {"min_edge": 0.75, "max_edge": 2.0, "rounds": 16, "depth_tolerance": 0.01, "views_per_batch": None}
    for bad, what in ((on + ["--mesh_collapse", "-1"], "min_edge"), (on + ["--mesh_collapse", "1", "--mesh_collapse_max_edge", "1"], "2 min_edge"),
                      (base + ["--mesh_collapse", "1"], "--mesh_collapse needs --mesh")):
        with pytest.raises(SystemExit):
            predict.parse_args(bad)
        assert what in capsys.readouterr().err
    assert "mesh_collapse_s" in open(predict.__file__).read()


def test_the_header_carries_the_entry_point_and_abi_11():
    from deep3d_aerial_amd import _lib, collapse

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    assert re.search(r"\bd3d_mesh_collapse_candidates\(", text) and "d3d_mesh_collapse_candidates" in _lib.SIGNATURES
    assert "mesh_collapse.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "does not claim to match" in collapse.__doc__ and "a setting, not a measurement" in collapse.__doc__
    # the validity tests are the decimation's own: one copy, in the shared header
    shared = open(os.path.join(_lib.CSRC, "geom_shared.h")).read()
    for name in ("dq_normal", "dq_shared", "dq_flips"):
        assert len(re.findall(r"\b%s\(const" % name, shared)) == 1
        for src in ("mesh_decimate.hip", "mesh_collapse.hip"):
            assert not re.search(r"\b%s\(const" % name, open(os.path.join(_lib.CSRC, src)).read()), (name, src)
    source = open(os.path.join(_lib.CSRC, "mesh_collapse.hip")).read()
    assert "dq_flips(" in source and "dq_shared(" in source and not re.search(r"atomic[A-Z]", source)


def test_the_bench_tools_torch_comparator_equals_the_restatement():
    """tools/mesh_collapse_bench.py's fp64 torch candidates, on CPU tensors, against candidates_numpy on two rounds of the scene."""
    import sys

    import torch

    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import mesh_collapse_bench as B

    s = scene()
    for d in (s["detail"][0], s["detail"][5]):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        topo = {"offset": t(d["offset"]), "nbr": t(d["nbr"]), "fixed": t(d["fixed"]), "face_offset": t(d["face_offset"]),
                "face_index": t(d["face_index"])}
        v, f = (s["V"], s["F"]) if d is s["detail"][0] else (s["detail"][4]["vertices"], s["detail"][4]["faces"])
        target, key = B.torch_candidates(t(v), t(f), topo, t(d["edges"]), t(d["measure"]), CS.MIN_EDGE, CS.MAX_EDGE)
        assert np.array_equal(key.numpy(), d["key"]) and np.array_equal(target.numpy().view(np.uint32), d["target"].view(np.uint32))
        assert (d["key"] >= 0).sum() > 100
    # the sliver share: 45 degrees, atan(1 / 10) = 5.7 degrees, and a face of no area, which counts
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [2, 0, 0]], np.float32)
    F = np.array([[0, 1, 2], [0, 3, 2], [0, 1, 4]], np.int32)
    share = lambda deg: B.sliver_share(torch.from_numpy(V), torch.from_numpy(F), deg)
    assert share(5.0) == 1 / 3 and share(10.0) == 2 / 3 and share(44.0) == 2 / 3 and share(46.0) == 1.0
