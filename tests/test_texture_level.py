"""Seam levelling of the texture on the CPU: a numpy restatement of the rules in deep3d_aerial_amd/texture.py (nodes, seam pairs,
smoothness edges, samples, right-hand side, the conjugate gradients, coverage and apply; tests/test_texture_level_gpu.py compares
the kernels with it), a dense fp64 solve, and hand-built cases."""
import os
import re

import numpy as np
import pytest

import test_texture as T

EMPTY = T.EMPTY
SMOOTH, ANCHOR = 0.1, 1e-3


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def level_graph_numpy(faces, chart, n_vertices, smooth=SMOOTH):
    """{"nodes" [N] int64 = chart * n + vertex (increasing), "face_nodes" [m, 3], "seams" / "smooth" [.] int64 = (i << 32) | j with
    i < j (distinct, increasing), "row_ptr", "column", "weight"}."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    chart = np.asarray(chart, np.int64)
    n = max(int(n_vertices), 1)
    m = len(F)
    has = chart >= 0
    nodes = np.unique((chart[has][:, None] * n + F[has]).ravel()) if has.any() else np.zeros(0, np.int64)
    index = {int(k): i for i, k in enumerate(nodes)}
    face_nodes = np.full((m, 3), -1, np.int32)
    for f in np.flatnonzero(has):
        face_nodes[f] = [index[int(chart[f] * n + v)] for v in F[f]]
    by_edge = {}
    for f in range(m):   # every face, with or without a winner
        for e in T.face_edges(F[f]):
            by_edge.setdefault(e, []).append(f)
    seams = set()
    for (a, b), fs in by_edge.items():
        if len(fs) != 2 or chart[fs[0]] < 0 or chart[fs[1]] < 0 or chart[fs[0]] == chart[fs[1]]:
            continue
        c1, c2 = sorted((int(chart[fs[0]]), int(chart[fs[1]])))
        for v in (a, b):
            seams.add((index[c1 * n + v] << 32) | index[c2 * n + v])
    smooths = set()
    for f in np.flatnonzero(has):
        for a, b in T.face_edges(face_nodes[f]):
            smooths.add((a << 32) | b)
    seams, smooths = np.array(sorted(seams), np.int64), np.array(sorted(smooths), np.int64)
    both = np.concatenate([seams, smooths])
    entry = np.sort(np.concatenate([both, ((both & 0xffffffff) << 32) | (both >> 32)]))
    row, col = entry >> 32, entry & 0xffffffff
    N = len(nodes)
    row_ptr = np.searchsorted(row, np.arange(N + 1)).astype(np.int32)
    node_chart = nodes // n
    weight = np.where(node_chart[row] != node_chart[col], np.float32(1.0), np.float32(smooth)).astype(np.float32)
    return {"n": n, "nodes": nodes, "face_nodes": face_nodes, "seams": seams, "smooth": smooths, "row_ptr": row_ptr,
            "column": col.astype(np.int32), "weight": weight}


def stack_pages(pages):
    """The pages as one [rows, P, 3] array, as the atlas the kernels see."""
    return np.concatenate([np.asarray(p) for p in pages], 0)


def split_rows(atlas, packing):
    return [atlas[packing.page_row[k]:packing.page_row[k + 1]] for k in range(packing.n_pages)]


def _vertex_uv(view, X):
    _, _, u, w = T.project(view, np.asarray(X, np.float32).astype(np.float64))
    return u, w


def level_samples_numpy(vertices, graph, rects, packing, chart_ids, views, atlas):
    """f [N, 3] fp32: the fp64 bilinear tap of atlas [rows, P, 3] at every node, rounded."""
    by_id = {v["id"]: v for v in views}
    n, nodes = graph["n"], graph["nodes"]
    f = np.zeros((len(nodes), 3), np.float32)
    A = atlas.astype(np.float64)
    for i, k in enumerate(nodes):
        ch, v = int(k // n), int(k % n)
        x0, y0, x1, y1 = (int(t) for t in rects[ch])
        page, ox, oy = (int(t) for t in packing.place[ch])
        u, w = _vertex_uv(by_id[int(chart_ids[ch])], np.asarray(vertices)[v][None])
        x = (u[0] - x0) + ox
        y = ((w[0] - y0) + oy) + float(packing.page_row[page])
        xf, yf = np.floor(x), np.floor(y)
        tx, ty = x - xf, y - yf
        row0 = int(packing.page_row[page]) + oy
        ix0 = int(min(max(xf, ox), ox + (x1 - x0)))
        iy0 = int(min(max(yf, row0), row0 + (y1 - y0)))
        ix1, iy1 = min(ix0 + 1, ox + (x1 - x0)), min(iy0 + 1, row0 + (y1 - y0))
        w00, w10, w01, w11 = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
        f[i] = (((w00 * A[iy0, ix0] + w10 * A[iy0, ix1]) + w01 * A[iy1, ix0]) + w11 * A[iy1, ix1]).astype(np.float32)
    return f


def rhs_numpy(graph, f):
    """b [N, 3] fp32: per row the sum, in column order, of f[j] - f[i] over its seam entries."""
    f = np.asarray(f, np.float32)
    node_chart = graph["nodes"] // graph["n"]
    b = np.zeros_like(f)
    for i in range(len(f)):
        s = np.zeros(3, np.float32)
        for e in range(graph["row_ptr"][i], graph["row_ptr"][i + 1]):
            j = graph["column"][e]
            if node_chart[j] != node_chart[i]:
                s = s + (f[j] - f[i])
        b[i] = s
    return b


def dense_matrix(graph, anchor=ANCHOR, dtype=np.float64):
    """(L + anchor I) [N, N]."""
    N = len(graph["nodes"])
    A = np.zeros((N, N), dtype)
    row = np.repeat(np.arange(N), np.diff(graph["row_ptr"]))
    A[row, graph["column"]] = -graph["weight"].astype(dtype)
    A[np.arange(N), np.arange(N)] = -A.sum(1) + dtype(anchor)
    return A


def dense_solve(graph, b, anchor=ANCHOR):
    if not len(b):
        return np.zeros((0, 3))
    return np.linalg.solve(dense_matrix(graph, anchor), np.asarray(b, np.float64))


def cg_numpy(graph, b, anchor=ANCHOR, tolerance=1e-4, iterations=500):
    """(g [N, 3] fp32, iterations, converged): the kernels' iteration on fp32 vectors with fp64 dot products: q = A r + beta q,
    p = r + beta p, alpha = rr / p.q, x += alpha p, r -= alpha q, beta = rr_new / rr; a channel that met |r| <= tolerance |b| is
    frozen (alpha = beta = 0)."""
    N = len(b)
    W = -dense_matrix(graph, 0.0, np.float32)
    np.fill_diagonal(W, 0.0)
    deg = np.zeros(N, np.float32)
    for i in range(N):
        for e in range(graph["row_ptr"][i], graph["row_ptr"][i + 1]):
            deg[i] = deg[i] + graph["weight"][e]
    dm = (deg + np.float32(anchor))[:, None]
    dot = lambda a, c: (a.astype(np.float64) * c.astype(np.float64)).sum(0)
    x = np.zeros((N, 3), np.float32)
    r = np.asarray(b, np.float32).copy()
    p, q = np.zeros_like(r), np.zeros_like(r)
    rr = dot(r, r)
    bb = rr.copy()
    tol2 = tolerance * tolerance
    done = rr <= tol2 * bb
    beta = np.zeros(3, np.float32)
    it = 0
    while not done.all() and it < iterations:
        q = (dm * r - W @ r) + beta * q
        p = r + beta * p
        pq = dot(p, q)
        with np.errstate(all="ignore"):
            alpha = np.where(done | ~(pq > 0), 0.0, rr / pq).astype(np.float32)
        x = x + alpha * p
        r = r - alpha * q
        t = dot(r, r)
        it += 1
        for c in range(3):
            if done[c]:
                beta[c] = 0.0
                continue
            beta[c] = np.float32(t[c] / rr[c])
            rr[c] = t[c]
            if t[c] <= tol2 * bb[c]:
                done[c], beta[c] = True, 0.0
    return x, it, bool(done.all())


def closest_numpy(X, Y, px, py):
    """(d2, w [.., 3]) of the points (px, py) to the triangle (X, Y)[0..2] in fp64: the kernels' regions in their order."""
    abx, aby, acx, acy = X[1] - X[0], Y[1] - Y[0], X[2] - X[0], Y[2] - Y[0]
    apx, apy = px - X[0], py - Y[0]
    d1, d2 = abx * apx + aby * apy, acx * apx + acy * apy
    bpx, bpy = px - X[1], py - Y[1]
    d3, d4 = abx * bpx + aby * bpy, acx * bpx + acy * bpy
    cpx, cpy = px - X[2], py - Y[2]
    d5, d6 = abx * cpx + aby * cpy, acx * cpx + acy * cpy
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    with np.errstate(all="ignore"):
        v_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        v_in, t_in = vb * den, vc * den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    w0 = np.select(conds, [one, zero, 1.0 - v_ab, zero, 1.0 - t_ac, zero], (1.0 - v_in) - t_in)
    w1 = np.select(conds, [zero, one, v_ab, zero, zero, 1.0 - t_bc], v_in)
    w2 = np.select(conds, [zero, zero, zero, one, t_ac, t_bc], t_in)
    inside = ~np.any(conds, 0)
    with np.errstate(all="ignore"):
        qx, qy = (w0 * X[0] + w1 * X[1]) + w2 * X[2], (w0 * Y[0] + w1 * Y[1]) + w2 * Y[2]
        dx, dy = px - qx, py - qy
        dist = dx * dx + dy * dy
    ok = np.isfinite(w0) & np.isfinite(w1) & np.isfinite(w2)
    dist = np.where(inside, np.where(ok, 0.0, np.inf), dist)
    return dist, np.stack([w0, w1, w2], -1)


def _face_texels(vertices, faces, f, view, rect, place):
    u, w = _vertex_uv(view, np.asarray(vertices)[np.asarray(faces[f], np.int64)])
    return (u - float(rect[0])) + float(place[1]), (w - float(rect[1])) + float(place[2])


def coverage_numpy(vertices, faces, chart, rects, packing, chart_ids, views):
    """cover [rows, P] int64: per texel the smallest (bits(fp32(d2)) << 32) | face over the faces of the rect's chart with
    d2 <= 2; EMPTY elsewhere."""
    by_id = {v["id"]: v for v in views}
    cover = np.full((int(packing.page_row[-1]), packing.page_size), EMPTY, np.int64)
    for f in np.flatnonzero(np.asarray(chart) >= 0):
        ch = int(chart[f])
        x0, y0, x1, y1 = (int(t) for t in rects[ch])
        page, ox, oy = (int(t) for t in packing.place[ch])
        X, Y = _face_texels(vertices, faces, f, by_id[int(chart_ids[ch])], rects[ch], packing.place[ch])
        bx0, bx1 = max(np.floor(X.min()) - 2, ox), min(np.ceil(X.max()) + 2, ox + (x1 - x0))
        by0, by1 = max(np.floor(Y.min()) - 2, oy), min(np.ceil(Y.max()) + 2, oy + (y1 - y0))
        if bx1 < bx0 or by1 < by0:
            continue
        ty, tx = np.mgrid[int(by0):int(by1) + 1, int(bx0):int(bx1) + 1]
        d2, _ = closest_numpy(X, Y, tx.astype(np.float64), ty.astype(np.float64))
        with np.errstate(invalid="ignore"):
            cand = d2 <= 2.0
        key = (np.where(cand, d2, 0.0).astype(np.float32).view(np.uint32).astype(np.int64) << 32) | np.int64(f)
        rows = int(packing.page_row[page]) + ty
        cover[rows[cand], tx[cand]] = np.minimum(cover[rows[cand], tx[cand]], key[cand])
    return cover


def apply_numpy(vertices, faces, chart, graph, g, cover, rects, packing, chart_ids, views, atlas):
    """The levelled atlas [rows, P, 3] uint8."""
    by_id = {v["id"]: v for v in views}
    g = np.asarray(g, np.float32)
    out = atlas.copy()
    rows, cols = np.nonzero(cover != EMPTY)
    face = (cover[rows, cols] & 0xffffffff).astype(np.int64)
    for f in np.unique(face):
        on = face == f
        ch = int(chart[f])
        page = int(packing.place[ch][0])
        X, Y = _face_texels(vertices, faces, f, by_id[int(chart_ids[ch])], rects[ch], packing.place[ch])
        _, w = closest_numpy(X, Y, cols[on].astype(np.float64), (rows[on] - int(packing.page_row[page])).astype(np.float64))
        w = w.astype(np.float32)
        g0, g1, g2 = (g[k][None, :3] for k in graph["face_nodes"][f])
        corr = (w[:, 0:1] * g0 + w[:, 1:2] * g1) + w[:, 2:3] * g2
        out[rows[on], cols[on]] = np.clip(np.rint(atlas[rows[on], cols[on]].astype(np.float32) + corr), 0, 255).astype(np.uint8)
    return out


def layout_numpy(vertices, faces, key, views, page_size=256, pad=2):
    from deep3d_aerial_amd import texture

    chart, labels = T.charts_numpy(faces, key)
    rects = T.rects_numpy(vertices, faces, key, chart, len(labels), views, pad)
    packing = texture.pack(rects, page_size)
    ids = (key[labels] & 0xffffffff).astype(np.int64)
    return chart, labels, rects, packing, ids


def seam_step(graph, f):
    """The mean absolute colour difference between the two sides' taps over all seam pairs (and channels)."""
    i, j = graph["seams"] >> 32, graph["seams"] & 0xffffffff
    return float(np.abs(np.asarray(f, np.float64)[i] - np.asarray(f, np.float64)[j]).mean())


def level_numpy(vertices, faces, key, views, page_size=256, pad=2, smooth=SMOOTH, anchor=ANCHOR, solve="dense", tolerance=1e-4,
                iterations=500):
    """The whole chain on the pages of T.atlas_numpy: {"graph", "f", "b", "g", "cover", "atlas" (unlevelled), "levelled", ...}."""
    chart, labels, rects, packing, ids = layout_numpy(vertices, faces, key, views, page_size, pad)
    atlas = stack_pages(T.atlas_numpy(rects, packing, ids, views))
    graph = level_graph_numpy(faces, chart, len(vertices), smooth)
    f = level_samples_numpy(vertices, graph, rects, packing, ids, views, atlas)
    b = rhs_numpy(graph, f)
    g = dense_solve(graph, b, anchor) if solve == "dense" else cg_numpy(graph, b, anchor, tolerance, iterations)[0]
    cover = coverage_numpy(vertices, faces, chart, rects, packing, ids, views)
    levelled = apply_numpy(vertices, faces, chart, graph, g, cover, rects, packing, ids, views, atlas)
    return {"chart": chart, "labels": labels, "rects": rects, "packing": packing, "ids": ids, "atlas": atlas, "graph": graph, "f": f,
            "b": b, "g": g, "cover": cover, "levelled": levelled}


# ----------------------------------------------------------------------------------------
# hand-built cases
# ----------------------------------------------------------------------------------------
def pairs(keys):
    return [(int(k >> 32), int(k & 0xffffffff)) for k in keys]


def test_two_triangles_across_one_seam_meet_the_closed_form():
    F = [[0, 1, 2], [1, 0, 3]]
    gr = level_graph_numpy(F, [0, 1], 4)
    assert list(gr["nodes"]) == [0, 1, 2, 4, 5, 7]   # (chart 0: a b c), (chart 1: a b d)
    assert pairs(gr["seams"]) == [(0, 3), (1, 4)]
    assert pairs(gr["smooth"]) == [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5)]
    assert list(gr["row_ptr"]) == [0, 3, 6, 8, 11, 14, 16] and list(gr["column"][:3]) == [1, 2, 3]
    assert list(gr["weight"][:3]) == [np.float32(SMOOTH), np.float32(SMOOTH), 1.0]
    for lam, mu, D in ((0.1, 1e-3, 40.0), (0.5, 0.25, -7.0), (2.0, 1e-2, 1.0)):
        gr = level_graph_numpy(F, [0, 1], 4, lam)
        gr["weight"] = gr["weight"].astype(np.float64)
        gr["weight"][gr["weight"] != 1.0] = lam   # the closed form is for lambda itself, not fp32(lambda)
        f = np.array([[10.0] * 3] * 3 + [[10.0 + D] * 3] * 3)
        b = rhs_numpy(gr, f)
        assert np.array_equal(b[:, 0], [D, D, 0, -D, -D, 0])
        g = dense_solve(gr, b, mu)[:, 0]
        s = D / (2 + mu + lam * mu / (2 * lam + mu))
        t = 2 * lam * s / (2 * lam + mu)
        assert np.allclose(g, [s, s, t, -s, -s, -t], rtol=1e-12, atol=0)


def test_a_vertex_where_three_charts_meet_gives_three_seam_pairs():
    F = [[0, 1, 2], [0, 2, 3], [0, 3, 1]]
    gr = level_graph_numpy(F, [0, 1, 2], 4)
    n = 4
    at_centre = [(i, j) for i, j in pairs(gr["seams"]) if gr["nodes"][i] % n == 0]
    assert len(at_centre) == 3 and len(gr["seams"]) == 6
    assert sorted((int(gr["nodes"][i] // n), int(gr["nodes"][j] // n)) for i, j in at_centre) == [(0, 1), (0, 2), (1, 2)]


def test_a_non_manifold_edge_and_an_edge_next_to_a_face_without_a_winner_give_no_seam():
    gr = level_graph_numpy([[0, 1, 2], [1, 0, 3], [0, 1, 4]], [0, 1, 2], 5)
    assert len(gr["seams"]) == 0 and len(gr["nodes"]) == 9
    gr = level_graph_numpy([[0, 1, 2], [1, 0, 3]], [0, -1], 4)
    assert len(gr["seams"]) == 0 and len(gr["nodes"]) == 3 and list(gr["face_nodes"][1]) == [-1, -1, -1]
    # the third face has no winner: the edge has three faces, still no seam between the other two
    gr = level_graph_numpy([[0, 1, 2], [1, 0, 3], [0, 1, 4]], [0, 1, -1], 5)
    assert len(gr["seams"]) == 0
    assert len(level_graph_numpy(np.zeros((0, 3), np.int32), np.zeros(0, np.int32), 0)["nodes"]) == 0


def _flat_views(colours, **kw):
    vs = []
    for k, c in enumerate(colours):
        v = T.cam_view(k + 1, **kw)
        v["image"] = np.empty(v["image"].shape, np.uint8)
        v["image"][...] = c
        vs.append(v)
    return vs


def test_one_chart_only_leaves_the_pages_as_they_are():
    V, F = T.strip(4)
    vs = _flat_views([(90, 120, 30)])
    key = np.full(len(F), T.make_key(1.0, 1), np.int64)
    res = level_numpy(V, F, key, vs, page_size=64)
    assert len(res["labels"]) == 1 and len(res["graph"]["seams"]) == 0
    assert not res["b"].any() and not res["g"].any()
    assert (res["cover"] != EMPTY).any() and np.array_equal(res["levelled"], res["atlas"])


def test_two_views_of_different_brightness_meet_in_the_middle():
    V, F = T.strip(6)
    vs = _flat_views([(100, 100, 100), (140, 60, 100)])
    key = np.where(np.arange(len(F)) < 6, T.make_key(1.0, 1), T.make_key(1.0, 2)).astype(np.int64)
    res = level_numpy(V, F, key, vs, page_size=64)
    gr = res["graph"]
    assert len(res["labels"]) == 2 and len(gr["seams"]) == 2
    before = seam_step(gr, res["f"])
    after = seam_step(gr, level_samples_numpy(V, gr, res["rects"], res["packing"], res["ids"], vs, res["levelled"]))
    assert before == pytest.approx(80 / 3) and after < 1.0
    # the blue channel agrees already: it is left alone; the conjugate gradients agree with the dense solve
    assert not res["g"][:, 2].any() and np.array_equal(res["levelled"][..., 2], res["atlas"][..., 2])
    g, it, ok = cg_numpy(gr, res["b"], tolerance=1e-6)
    assert ok and it < 100 and np.abs(g - res["g"]).max() < 1e-2


# texel coordinates: cam_view(f=40) maps x to u = 31.5 + 4 x and y to v = 23.5 + 4 y on z = 10, exactly
def _at(u, v):
    return [(u - 31.5) / 4.0, (v - 23.5) / 4.0, 10.0]


def test_coverage_on_a_shared_edge_at_the_bound_and_beyond():
    V = np.array([_at(34, 26), _at(38, 26), _at(34, 30), _at(38, 30)], np.float32)
    F = np.array([[0, 2, 1], [1, 2, 3]], np.int32)
    vs = [T.cam_view(1)]
    key = np.full(2, T.make_key(1.0, 1), np.int64)
    chart, labels, rects, packing, ids = layout_numpy(V, F, key, vs, 64, 2)
    assert list(rects[0]) == [32, 24, 40, 32] and list(packing.place[0]) == [0, 2, 0]
    cover = coverage_numpy(V, F, chart, rects, packing, ids, vs)
    at = lambda u, v: int(cover[v - 24, u - 32 + 2])
    zero, two = 0, int(np.float32(2.0).view(np.uint32)) << 32
    for u, v in ((36, 28), (37, 27), (35, 29)):   # centres on the shared edge: both faces at d2 = 0, the lower index wins
        assert at(u, v) == zero | 0
    assert at(35, 27) == zero | 0 and at(37, 29) == zero | 1
    assert at(33, 25) == two | 0    # one texel out along the diagonal of corner (34, 26): d2 = 2, covered
    assert at(39, 31) == two | 1
    assert at(32, 24) == EMPTY and at(32, 26) == EMPTY and at(33, 24) == EMPTY   # the next ones out are not
    assert at(33, 26) == (int(np.float32(1.0).view(np.uint32)) << 32) | 0
    # apply: a covered texel moves by the correction at its closest point, an uncovered one keeps its colour
    gr = level_graph_numpy(F, chart, 4)
    g = np.float32([[10, 0, 0], [20, 0, 0], [40, 0, 0], [80, 0, 0]])
    atlas = np.full((int(packing.page_row[-1]), 64, 3), 100, np.uint8)
    out = apply_numpy(V, F, chart, gr, g, cover, rects, packing, ids, vs, atlas)
    px = lambda u, v: int(out[v - 24, u - 32 + 2, 0])
    assert px(33, 25) == 110 and px(34, 26) == 110 and px(38, 26) == 120 and px(39, 31) == 180
    assert px(36, 28) == 130 and px(36, 26) == 115   # midpoints of edges: the mean of their ends
    assert px(32, 24) == 100 and (out[..., 1:] == 100).all()
    assert apply_numpy(V, F, chart, gr, g * 100, cover, rects, packing, ids, vs, atlas).max() == 255


def test_coverage_never_leaves_the_charts_rect():
    V, F = T.strip(6)
    vs = _flat_views([(100, 100, 100), (140, 60, 100)])
    key = np.where(np.arange(len(F)) < 6, T.make_key(1.0, 1), T.make_key(1.0, 2)).astype(np.int64)
    chart, labels, rects, packing, ids = layout_numpy(V, F, key, vs, 64, 1)
    assert packing.place[0][2] == packing.place[1][2] and packing.place[1][1] == packing.place[0][1] + rects[0][2] - rects[0][0] + 1
    cover = coverage_numpy(V, F, chart, rects, packing, ids, vs)
    for ch in range(2):
        page, ox, oy = (int(t) for t in packing.place[ch])
        w, h = rects[ch][2] - rects[ch][0] + 1, rects[ch][3] - rects[ch][1] + 1
        part = cover[oy:oy + h, ox:ox + w]
        faces_here = part[part != EMPTY] & 0xffffffff
        assert len(faces_here) and (chart[faces_here] == ch).all()
    covered = cover != EMPTY
    covered[:, 2:packing.place[1][1] + rects[1][2] - rects[1][0] + 1] = False
    assert not covered.any()


def test_argument_errors_of_the_level_settings():
    from deep3d_aerial_amd import texture

    base = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in (["--level_smooth", "-0.1"], ["--level_anchor", "0"], ["--level_anchor", "-1"], ["--level_tolerance", "0"],
                ["--level_tolerance", "1"], ["--level_iterations", "0"]):
        for flags in (bad, ["--level"] + bad):
            with pytest.raises(SystemExit):
                texture.main(base + flags)
    assert texture.check_level_settings({}) == (0.1, 1e-3, 1e-4, 500)
    assert texture.check_settings({}) == (0.01, None, 8192, 2)
    for bad in ({"smooth": -1}, {"anchor": 0}, {"tolerance": 1.5}, {"iterations": 0}, {"iterations": 2.5}):
        with pytest.raises(ValueError):
            texture.check_level_settings(bad)


def test_predict_turns_texture_level_flags_into_the_stages_settings():
    from deep3d_aerial_amd import predict

    base = ["--output_folder", "out", "--synthetic_items", "2", "--random_weights", "--fuse", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.5",
            "--texture", "t.ply"]
    assert predict._texture_settings(predict.parse_args(base))["level"] is None
    a = predict.parse_args(base + ["--texture_level", "--texture_level_smooth", "0.5", "--texture_level_iterations", "40"])
    assert predict._texture_settings(a)["level"] == {"smooth": 0.5, "anchor": 1e-3, "tolerance": 1e-4, "iterations": 40}
    for bad in (["--texture_level_anchor", "0"], ["--texture_level", "--texture_level_tolerance", "2"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    names = [n for n in _lib.SIGNATURES if n.startswith("d3d_texture_level_")]
    assert "d3d_texture_level_scratch_bytes" in names and len(names) == 8
    for n in names:
        assert re.search(r"\b%s\(" % n, text), n
    src = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "texture_level.hip" in src
