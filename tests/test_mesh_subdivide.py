"""The subdivision of the surface mesh restated in numpy from the rule's text (deep3d_aerial_amd/subdivide.py),
and that restatement checked on its own: hand-worked templates, areas and normals, closedness and boundary loops, invariance under
face permutation and corner rotation, view order and batching, the fixed point after an early stop; settings, command-line errors,
header and binding.  tests/test_mesh_subdivide_gpu.py holds the kernels to it bit for bit."""
import os
import re

import numpy as np
import pytest

import mesh_subdivide_scene as SS

NAMES = ("d3d_mesh_subdivide_measure", "d3d_mesh_subdivide_scratch_bytes", "d3d_mesh_subdivide_plan", "d3d_mesh_subdivide_emit")
_SCENE = {}


# ----------------------------------------------------------------------------------------
# the rule in numpy
# ----------------------------------------------------------------------------------------
def edges_numpy(F):
    """Rule 2: the undirected edges a < b in (a, b) lexicographic order, [E, 2] int32."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1)
    return np.unique(e, axis=0).astype(np.int32).reshape(-1, 2)


def seen_numpy(view, X, tol):
    """(seen [k] bool, u, v [k] fp64) of the points X [k, 3] (fp64) in one view: ortho's candidate test."""
    K, E = np.asarray(view["K"], np.float64), np.asarray(view["E"], np.float64)
    R, t = E[:3, :3], E[:3, 3]
    D = np.asarray(view["depth"], np.float32)
    H, W = D.shape
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        p = [((R[r, 0] * X0 + R[r, 1] * X1) + R[r, 2] * X2) + t[r] for r in range(3)]
        q = [(K[r, 0] * p[0] + K[r, 1] * p[1]) + K[r, 2] * p[2] for r in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        ok = (p[2] > 0) & (q[2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        px = np.where(ok, np.floor(u + 0.5), 0).astype(np.int64)
        py = np.where(ok, np.floor(v + 0.5), 0).astype(np.int64)
        d = D[py, px]
        ok &= np.isfinite(d) & (d > 0) & (p[2] <= d.astype(np.float64) * (1.0 + tol))
    return ok, u, v


def edge_l2_numpy(view, V, E, tol=SS.TOLERANCE):
    """Per edge the view's l2, or -1 where the view does not see both ends or l2 is not finite."""
    V = np.asarray(V, np.float32).astype(np.float64)
    sa, ua, va = seen_numpy(view, V[E[:, 0]], tol)
    sb, ub, vb = seen_numpy(view, V[E[:, 1]], tol)
    with np.errstate(all="ignore"):
        du, dv = ua - ub, va - vb
        l2 = du * du + dv * dv
    return np.where(sa & sb & np.isfinite(l2), l2, -1.0)


def measure_numpy(V, E, views, tol=SS.TOLERANCE, measure=None):
    """Rule 3: the largest l2 over the views, max-merged into `measure`."""
    m = np.zeros(len(E), np.float64) if measure is None else measure.copy()
    for view in views:
        l2 = edge_l2_numpy(view, V, E, tol)
        m = np.where(l2 > m, l2, m)
    return m


def plan_numpy(V, F, E, measure, max_edge):
    """Rules 4 and 5's counts: mark, rank, midpoint, face_edge, child_count, child_offset, totals."""
    V = np.asarray(V, np.float32)
    a, b = V[E[:, 0]], V[E[:, 1]]
    mid = ((a.astype(np.float64) + b.astype(np.float64)) * 0.5).astype(np.float32)
    mark = (measure > float(max_edge) * float(max_edge)) & (mid != a).any(1) & (mid != b).any(1)
    mark = mark.astype(np.int32)
    rank = (np.cumsum(mark) - mark).astype(np.int32)
    index = {(int(x), int(y)): k for k, (x, y) in enumerate(E)}
    fe = np.array([[index[(min(f[i], f[(i + 1) % 3]), max(f[i], f[(i + 1) % 3]))] for i in range(3)] for f in F.tolist()], np.int32).reshape(-1, 3)
    count = (1 + mark[fe].sum(1)).astype(np.int32) if len(F) else np.zeros(0, np.int32)
    offset = (np.cumsum(count) - count).astype(np.int32)
    return {"mark": mark, "rank": rank, "midpoint": mid, "face_edge": fe, "child_count": count, "child_offset": offset,
            "totals": np.array([mark.sum(), count.sum()], np.int64)}


def _d2(x, y):
    d = x.astype(np.float64) - y.astype(np.float64)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def emit_numpy(V, F, p):
    """Rules 5 and 6: (vertices, faces) after the split."""
    V = np.asarray(V, np.float32)
    n = len(V)
    out_v = np.concatenate([V, p["midpoint"][p["mark"] != 0]]).astype(np.float32)
    out_f = []
    for f, fe in zip(F.tolist(), p["face_edge"].tolist()):
        m = [n + int(p["rank"][e]) if p["mark"][e] else -1 for e in fe]
        k = sum(x >= 0 for x in m)
        if k == 0:
            out_f.append(f)
        elif k == 1:
            i = [x >= 0 for x in m].index(True)
            a, b, c = f[i], f[(i + 1) % 3], f[(i + 2) % 3]
            out_f += [[a, m[i], c], [m[i], b, c]]
        elif k == 2:
            i = [x >= 0 for x in m].index(False)
            j, l = (i + 1) % 3, (i + 2) % 3
            a, b, c, P, Q = f[i], f[j], f[l], m[j], m[l]
            out_f.append([P, c, Q])
            ap, bq = _d2(V[a], p["midpoint"][fe[j]]), _d2(V[b], p["midpoint"][fe[l]])
            through_a = ap < bq or (not bq < ap and a < b)
            out_f += [[a, b, P], [a, P, Q]] if through_a else [[a, b, Q], [b, P, Q]]
        else:
            out_f += [[f[0], m[0], m[2]], [m[0], f[1], m[1]], [m[2], m[1], f[2]], [m[0], m[1], m[2]]]
    return out_v, np.array(out_f, np.int32).reshape(-1, 3)


def subdivide_numpy(V, F, views, max_edge, rounds=SS.ROUNDS, tol=SS.TOLERANCE, detail=None):
    """Rule 7: (vertices, faces, stopped early); detail (a list) gets every round's passes."""
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int32)
    early = False
    for _ in range(rounds):
        E = edges_numpy(F)
        measure = measure_numpy(V, E, views, tol)
        p = plan_numpy(V, F, E, measure, max_edge)
        if detail is not None:
            detail.append(dict(p, edges=E, measure=measure, V=V, F=F))
        if p["totals"][0] == 0:
            early = True
            break
        V, F = emit_numpy(V, F, p)
        if detail is not None:
            detail[-1].update(out_v=V, out_f=F)
    return V, F, early


def scene():
    """The scene and its chain, computed once: V, F, cases, views, detail (per round), out_v, out_f, early."""
    if not _SCENE:
        views = SS.numpy_views()
        V, F, cases = SS.build(views)
        detail = []
        out_v, out_f, early = subdivide_numpy(V, F, views, SS.MAX_EDGE, detail=detail)
        _SCENE.update(V=V, F=F, cases=cases, views=views, detail=detail, out_v=out_v, out_f=out_f, early=early)
    return _SCENE


# ----------------------------------------------------------------------------------------
# helpers of the checks
# ----------------------------------------------------------------------------------------
def canonical(F):
    """Every face with its smallest index first (the winding kept), the rows sorted."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    k = F.argmin(1)
    G = np.stack([F[np.arange(len(F)), (k + i) % 3] for i in range(3)], 1)
    return G[np.lexsort((G[:, 2], G[:, 1], G[:, 0]))]


def area_vectors(V, F):
    V = np.asarray(V, np.float64)
    return 0.5 * np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])


def edge_use(F):
    """{undirected edge: number of faces}"""
    use = {}
    for f in np.asarray(F).tolist():
        for i in range(3):
            k = (min(f[i], f[(i + 1) % 3]), max(f[i], f[(i + 1) % 3]))
            use[k] = use.get(k, 0) + 1
    return use


def boundary_loops(F):
    """The number of cycles of boundary half-edges (every boundary vertex simple)."""
    use, nxt = edge_use(F), {}
    for f in np.asarray(F).tolist():
        for i in range(3):
            a, b = f[i], f[(i + 1) % 3]
            if use[(min(a, b), max(a, b))] == 1:
                assert a not in nxt
                nxt[a] = b
    loops, left = 0, set(nxt)
    while left:
        a = s = left.pop()
        while nxt[a] != s:
            a = nxt[a]
            left.discard(a)
        loops += 1
    return loops


def flat_view(f=100.0, size=201, depth=10.0, centre=(0.0, 0.0)):
    """A camera at (centre, 0) looking along +z at a constant depth map: a point (x, y, z) lands at u = f (x - cx) / z + c."""
    c = (size - 1) / 2.0
    K = np.array([[f, 0, c], [0, f, c], [0, 0, 1]], np.float64)
    E = np.eye(4)
    E[:3, 3] = (-centre[0], -centre[1], 0.0)
    return {"K": K, "E": E, "depth": np.full((size, size), depth, np.float32)}


def octahedron():
    V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return V, F


def grid(nx, ny, step=1.0, z=10.0):
    gx, gy = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
    V = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1).astype(np.float32)
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return V, np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, d], 1)]).astype(np.int32)


def _forced(V, F, split_edges):
    """plan and emit with the measure forced: the listed edges (pairs) are over the limit."""
    E = edges_numpy(F)
    want = {(min(a, b), max(a, b)) for a, b in split_edges}
    measure = np.array([100.0 if (int(a), int(b)) in want else 0.0 for a, b in E])
    p = plan_numpy(V, F, E, measure, 2.0)
    return p, emit_numpy(V, F, p)


# ----------------------------------------------------------------------------------------
# the restatement on its own
# ----------------------------------------------------------------------------------------
TRI_V = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], np.float32)   # edges: (0,1) -> 3, (0,2) -> 4, (1,2) -> 5 in list order when split


def test_hand_worked_templates():
    F = np.array([[0, 1, 2]], np.int32)
    assert edges_numpy(F).tolist() == [[0, 1], [0, 2], [1, 2]]
    p, (v, f) = _forced(TRI_V, F, [])
    assert f.tolist() == [[0, 1, 2]] and np.array_equal(v, TRI_V) and p["totals"].tolist() == [0, 1]
    # one edge, at every corner
    for rot, face in enumerate(([0, 1, 2], [2, 0, 1], [1, 2, 0])):   # e_rot = (0, 1)
        p, (v, f) = _forced(TRI_V, np.array([face], np.int32), [(0, 1)])
        assert p["face_edge"][0, rot] == 0 and v[3].tolist() == [4, 0, 0] and p["totals"].tolist() == [1, 2]
        assert f.tolist() == [[0, 3, 2], [3, 1, 2]]
    # two edges: (0, 1) stays; p = mid(1, 2) = 4 (rank 1), q = mid(2, 0) = 3 (rank 0).  |0 - p|^2 = 32 = |1 - q|^2... no: (4,4) from 0 is
    # 32, (0,4) from (8,0) is 80: a-p is shorter
    p, (v, f) = _forced(TRI_V, F, [(1, 2), (0, 2)])
    assert v[3].tolist() == [0, 4, 0] and v[4].tolist() == [4, 4, 0]
    assert f.tolist() == [[4, 2, 3], [0, 1, 4], [0, 4, 3]]
    # with the right angle at b the other diagonal is shorter
    Vb = np.array([[8, 0, 0], [0, 0, 0], [0, 8, 0]], np.float32)
    p, (v, f) = _forced(Vb, F, [(1, 2), (0, 2)])
    assert f.tolist() == [[4, 2, 3], [0, 1, 3], [1, 4, 3]]
    # an isosceles triangle ties: the diagonal starts at the smaller of a and b
    Vt = np.array([[-4, 0, 0], [4, 0, 0], [0, 16, 0]], np.float32)
    p, (v, f) = _forced(Vt, F, [(1, 2), (0, 2)])
    assert _d2(Vt[0], v[4]) == _d2(Vt[1], v[3]) and f.tolist() == [[4, 2, 3], [0, 1, 4], [0, 4, 3]]
    p, (v, f) = _forced(Vt[[1, 0, 2]], np.array([[1, 0, 2]], np.int32), [(1, 2), (0, 2)])   # a = 1, b = 0
    assert f.tolist() == [[3, 2, 4], [1, 0, 4], [0, 3, 4]]
    # three edges
    p, (v, f) = _forced(TRI_V, F, [(0, 1), (1, 2), (0, 2)])
    assert p["rank"].tolist() == [0, 1, 2] and p["totals"].tolist() == [3, 4]
    assert f.tolist() == [[0, 3, 4], [3, 1, 5], [4, 5, 2], [3, 5, 4]]


def test_new_indices_follow_the_edge_order_not_the_face_order():
    V, F = grid(3, 3)
    E = edges_numpy(F)
    split = [tuple(E[k]) for k in (1, 4, 7, 8, 12)]
    p, (v, f) = _forced(V, F, split)
    assert p["mark"].nonzero()[0].tolist() == [1, 4, 7, 8, 12] and p["rank"][[1, 4, 7, 8, 12]].tolist() == [0, 1, 2, 3, 4]
    perm = np.random.default_rng(3).permutation(len(F))
    p2, (v2, f2) = _forced(V, F[perm], split)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(canonical(f2), canonical(f))
    assert np.array_equal(p2["child_offset"], np.cumsum(p2["child_count"]) - p2["child_count"])


def test_child_areas_sum_to_the_parent_and_normals_keep_its_side():
    s = scene()
    for d in s["detail"]:
        if "out_f" not in d:
            continue
        parent = area_vectors(d["V"], d["F"])
        child = area_vectors(d["out_v"], d["out_f"])
        for k, (o, c) in enumerate(zip(d["child_offset"], d["child_count"])):
            total = child[o:o + c].sum(0)
            scale = max(np.abs(np.asarray(d["V"], np.float64)[d["F"][k]]).max(), 1.0) ** 2
            assert np.abs(total - parent[k]).max() <= 1e-5 * scale   # fp32 midpoints
            if np.linalg.norm(parent[k]) > 1e-3 * scale:
                assert (child[o:o + c] @ parent[k] > 0).all()
    # exactly, where the midpoints are exact
    V, F = grid(4, 3, step=2.0)
    p, (v, f) = _forced(V, F, [tuple(e) for e in edges_numpy(F)[::2]])
    child = area_vectors(v, f)
    for k, (o, c) in enumerate(zip(p["child_offset"], p["child_count"])):
        assert np.array_equal(child[o:o + c].sum(0), area_vectors(V, F)[k:k + 1][0]) and (child[o:o + c][:, 2] < 0).all()


def test_closed_stays_closed_and_boundary_loops_are_kept():
    V, F = octahedron()
    view = flat_view(f=40.0, depth=20.0)
    Vs = (V + np.array([0, 0, 5], np.float32)).astype(np.float32)
    v, f, early = subdivide_numpy(Vs, F, [view], 4.0, rounds=3, tol=10.0)   # the tolerance lets the far side count as seen
    assert len(f) > len(F) and set(edge_use(f).values()) == {2} and len(v) - len(edge_use(f)) + len(f) == 2
    V, F = grid(5, 4, step=1.0, z=10.0)
    F = F[[k for k in range(len(F)) if k not in (5, 5 + 12)]]   # a hole of two faces (one cell) inside
    view = flat_view(centre=(2.0, 1.5))
    assert boundary_loops(F) == 2
    v, f, early = subdivide_numpy(V, F, [view], 4.0, rounds=3)
    use = edge_use(f)
    assert len(f) > 4 * len(F) and set(use.values()) == {1, 2} and boundary_loops(f) == 2


def test_permuting_or_rotating_the_faces_gives_the_same_mesh():
    s = scene()
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(s["F"]))
    rot = rng.integers(0, 3, len(s["F"]))
    F2 = np.stack([s["F"][perm, (rot + i) % 3] for i in range(3)], 1).astype(np.int32)
    v2, f2, early = subdivide_numpy(s["V"], F2, s["views"], SS.MAX_EDGE)
    assert np.array_equal(v2.view(np.uint32), s["out_v"].view(np.uint32))
    assert np.array_equal(canonical(f2), canonical(s["out_f"])) and early == s["early"]


def test_the_measure_does_not_depend_on_view_order_or_batching():
    s = scene()
    d = s["detail"][0]
    V, E, vs = d["V"], d["edges"], s["views"]
    want = d["measure"]
    assert np.array_equal(measure_numpy(V, E, vs[::-1]), want)
    part = measure_numpy(V, E, vs[4:])
    assert not np.array_equal(part, want) and np.array_equal(measure_numpy(V, E, vs[:4], measure=part), want)
    m = None
    for k in range(0, len(vs), 2):
        m = measure_numpy(V, E, vs[k:k + 2], measure=m)
    assert np.array_equal(m, want) and np.array_equal(measure_numpy(V, E, vs, measure=want), want)
    assert not measure_numpy(V, E, []).any()


def core():
    """The scene's core (mesh_subdivide_scene.core_faces) and its chain, computed once: F, detail, out_v, out_f, early."""
    s = scene()
    if "core" not in s:
        F = SS.core_faces(s["V"], s["F"], s["cases"])
        detail = []
        out_v, out_f, early = subdivide_numpy(s["V"], F, s["views"], SS.MAX_EDGE, detail=detail)
        s["core"] = dict(F=F, detail=detail, out_v=out_v, out_f=out_f, early=early)
    return s["core"]


def test_after_an_early_stop_no_seen_edge_is_too_long():
    s, c = scene(), core()
    assert c["early"] and 2 <= len(c["detail"]) <= SS.ROUNDS and c["detail"][-1]["totals"][0] == 0 and len(c["out_f"]) > 16 * len(c["F"])
    E = edges_numpy(c["out_f"])
    m = measure_numpy(c["out_v"], E, s["views"])
    assert (m > 0).sum() > 1000 and not (m > SS.MAX_EDGE ** 2).any()
    # capped at one round the loop does not stop early and leaves long edges behind
    v1, f1, early1 = subdivide_numpy(s["V"], c["F"], s["views"], SS.MAX_EDGE, rounds=1)
    assert not early1 and np.array_equal(f1, c["detail"][0]["out_f"])
    assert (measure_numpy(v1, edges_numpy(f1), s["views"]) > SS.MAX_EDGE ** 2).sum() > 100
    # the whole scene is still splitting in its last round, and the edge between neighbouring floats stays over the limit unsplit
    assert not s["early"] and len(s["detail"]) == SS.ROUNDS and s["detail"][-1]["totals"][0] > 0
    E = edges_numpy(s["out_f"])
    k = E.tolist().index(sorted(s["cases"]["coincide"]))
    assert measure_numpy(s["out_v"], E[k:k + 1], s["views"])[0] > SS.MAX_EDGE ** 2


def test_the_scene_holds_every_crafted_case():
    s = scene()
    V, F, cases, views = s["V"], s["F"], s["cases"], s["views"]
    d = s["detail"][0]
    E, m, mark = d["edges"], d["measure"], d["mark"]
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(E)}
    eid = lambda a, b: index[(min(a, b), max(a, b))]
    lim = SS.MAX_EDGE ** 2
    per_view = np.stack([edge_l2_numpy(v, V, E) for v in views])
    # the grid: coarse (several times max_edge), every edge of it split, with a boundary
    g = cases["grid"]
    ge = [eid(int(g[j, i]), int(g[j, i + 1])) for j in range(g.shape[0]) for i in range(1, g.shape[1] - 1)]
    assert (np.sqrt(m[ge]) > 3 * SS.MAX_EDGE).all() and mark[ge].all()
    use = edge_use(F)
    assert 1 in use.values() and use[tuple(sorted(cases["three_faces"]))] == 3
    # the slanted patch: some edge is over the limit in one view that sees it and under it in another
    ps = set(cases["slanted"].ravel().tolist())
    pe = [k for k, (a, b) in enumerate(E) if int(a) in ps and int(b) in ps]
    disagree = [k for k in pe if ((per_view[:, k] > lim).any() and ((per_view[:, k] >= 0) & (per_view[:, k] <= lim)).any())]
    assert disagree and mark[disagree].all()
    # every template at every corner, both diagonals, and the tie on both sides
    want = {"none": 1, "one": 2, "two_ap": 3, "two_bq": 3, "two_tie_a": 3, "two_tie_b": 3, "three": 4}
    out_f = d["out_f"]
    for (name, rot), f in cases["hand"].items():
        fe = d["face_edge"][f]
        assert d["child_count"][f] == want[name], (name, rot)
        if name == "one":
            assert mark[fe].tolist() == [int(i == rot) for i in range(3)]
        if name.startswith("two"):
            assert mark[fe].tolist() == [int(i != rot) for i in range(3)]
            a, b = int(F[f][rot]), int(F[f][(rot + 1) % 3])
            P, Q = d["midpoint"][fe[(rot + 1) % 3]], d["midpoint"][fe[(rot + 2) % 3]]
            ap, bq = _d2(V[a], P), _d2(V[b], Q)
            second = out_f[d["child_offset"][f] + 1].tolist()
            through_a = second[2] == len(V) + d["rank"][fe[(rot + 1) % 3]]
            if name == "two_ap":
                assert ap < bq and through_a
            elif name == "two_bq":
                assert bq < ap and not through_a
            else:
                assert ap == bq and through_a == (a < b) == (name == "two_tie_a")
    # an unreferenced vertex, an edge with one end outside every image, a hidden edge, an edge whose midpoint is one of its ends
    assert cases["unreferenced"] not in set(F.ravel().tolist())
    a, b = cases["outside"]
    seen = [seen_numpy(v, V[[a, b]].astype(np.float64), SS.TOLERANCE)[0] for v in views]
    assert any(x[0] for x in seen) and not any(x[1] for x in seen) and m[eid(a, b)] == 0
    a, b = cases["hidden"]
    inside = [seen_numpy(v, V[[a, b]].astype(np.float64), 1e9)[0].all() for v in views]   # the depth test switched off
    assert any(inside) and m[eid(a, b)] == 0 and not mark[eid(a, b)]
    a, b = cases["coincide"]
    k = eid(a, b)
    assert m[k] > 100 * lim and not mark[k] and ((d["midpoint"][k] == V[a]).all() or (d["midpoint"][k] == V[b]).all())
    assert d["totals"][0] > 100 and len(s["out_f"]) > 16 * len(F)


# ----------------------------------------------------------------------------------------
# settings, command line, header
# ----------------------------------------------------------------------------------------
def test_settings_are_checked():
    from deep3d_aerial_amd import mesh, subdivide

    s = subdivide.check_subdivide_settings({"max_edge": 4})
    assert s == {"max_edge": 4.0, "rounds": 4, "depth_tolerance": 0.01, "views_per_batch": None}
    assert subdivide.check_subdivide_settings({"max_edge": 1, "rounds": 8, "depth_tolerance": 0, "views_per_batch": 2})["rounds"] == 8
    for bad in ({}, {"max_edge": None}, {"max_edge": 0.5}, {"max_edge": float("nan")}, {"max_edge": float("inf")}, {"max_edge": "x"},
                {"max_edge": 4, "rounds": 0}, {"max_edge": 4, "rounds": 9}, {"max_edge": 4, "rounds": 2.5},
                {"max_edge": 4, "depth_tolerance": -1}, {"max_edge": 4, "depth_tolerance": float("nan")},
                {"max_edge": 4, "views_per_batch": 0}, {"max_edge": 4, "reach": 1}):
        with pytest.raises(ValueError):
            subdivide.check_subdivide_settings(bad)
    with pytest.raises(ValueError, match="int32"):
        subdivide.check_sizes((1 << 31) - 10, 10, 5)
    with pytest.raises(ValueError, match="int32"):
        subdivide.check_sizes(10, 10, -(-(1 << 31) // 6))
    subdivide.check_sizes((1 << 31) - 11, 10, ((1 << 31) - 1) // 6)
    # the mesh settings carry it under "subdivide", with their own views_per_batch
    assert mesh.subdivide_settings({"views_per_batch": 3}) is None
    got = mesh.subdivide_settings({"views_per_batch": 3, "subdivide": {"max_edge": 5, "rounds": 2, "depth_tolerance": 0.02}})
    assert got == {"max_edge": 5.0, "rounds": 2, "depth_tolerance": 0.02, "views_per_batch": 3}
    for bad in ({"max_edge": 0}, {"rounds": 2}, {"max_edge": 4, "views_per_batch": 2}):
        with pytest.raises(ValueError):
            mesh.subdivide_settings({"subdivide": bad})


def test_the_flags_parse_and_clean_has_no_views(capsys):
    import argparse

    from deep3d_aerial_amd import mesh, predict, subdivide

    ap = argparse.ArgumentParser()
    mesh.add_arguments(ap, prefix="mesh_")
    base = ["--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.1"]
    a = ap.parse_args(base)
    assert "subdivide" not in mesh.settings_from_args(a, "m.ply", "mesh_")   # the key is carried only when the flag is given
    a = ap.parse_args(base + ["--mesh_subdivide", "6", "--mesh_subdivide_rounds", "2"])
    s = mesh.settings_from_args(a, "m.ply", "mesh_")
    assert s["subdivide"] == {"max_edge": 6.0, "rounds": 2, "depth_tolerance": subdivide.DEFAULT_TOLERANCE}
    mesh.check_args(ap, a, "mesh_")
    for bad in (["--mesh_subdivide", "0.5"], ["--mesh_subdivide", "4", "--mesh_subdivide_rounds", "9"]):
        with pytest.raises(SystemExit):
            mesh.check_args(ap, ap.parse_args(base + bad), "mesh_")
    assert "subdivide" in capsys.readouterr().err
    # the mesh tool: --clean has no views
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--out", "out.ply", "--subdivide", "4"])
    assert "--subdivide needs the views" in capsys.readouterr().err
    # the stand-alone tool
    tool = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in (tool, tool + ["--max_edge", "0"], tool + ["--max_edge", "4", "--rounds", "0"], tool + ["--max_edge", "4", "--depth_tolerance", "-1"],
                tool[:4] + ["--out", "o.obj", "--max_edge", "4"], tool + ["--max_edge", "4", "--views_per_batch", "0"]):
        with pytest.raises(SystemExit):
            subdivide.main(bad)
    capsys.readouterr()
    # predict knows the flags
    text = open(predict.__file__).read()
    assert "mesh_subdivide_s" in text


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib, subdivide

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in _lib.SIGNATURES, n
    assert "mesh_subdivide.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "does not claim to match" in subdivide.__doc__ and "a setting, not a measurement" in subdivide.__doc__
    source = open(os.path.join(_lib.CSRC, "mesh_subdivide.hip")).read()
    assert not re.search(r"atomic[A-Z]", source)   # no atomics of any kind
