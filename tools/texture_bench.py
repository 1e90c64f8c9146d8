"""The texturing kernels (csrc/texture.hip) at survey size: the meshes of tools/mesh_bench.py's scenes (0.5 m and 0.25 m voxels,
V = 32 and V = 128 views of 2752 x 1856) textured from the same views with synthetic images.  Device-event times of select,
charts, rects, fill (with the empty-colour pass) and texcoords; faces, charts, pages and candidate views per face; and a per-view
fp64 torch version of select, checked for the same keys.  The `level` entry times the seam levelling (csrc/texture_level.hip) on the
same atlas: graph, samples, solve (with its iteration count), coverage and apply, and beside the solve a torch restatement of the
same iteration (index_add per iteration) on the same graph, per iteration.  The `local` entry times the local seam levelling
(csrc/texture_local.hip) on the same atlas: seams and samples (with torch's sorts), the fold, the band alone, the solve (the band
and the sweeps, every repeat from a fresh copy of the folded state) with its sweep count and the share of charts and of texels on
each path, each path's charts alone, the LDS path's charts in one launch instead of three by LDS class, and apply; --no_local
skips it.  With
--smooth_views W every row gains a `smooth` entry
(csrc/texture_smooth.hip): the candidates pass beside select, the smoothing's time and rounds, the charts, pages and the rects and
fill times before and after, the mean and largest loss of projected area and the share of faces whose candidate list is full,
which is where 16 candidates truncate.  With --outlier_threshold T every row gains an `outliers` entry
(csrc/texture_outliers.hip): the colour pass and the vote on the row's candidate lists, the candidates pass of the same row beside
them, the summary counts, and a per-view fp64 torch version of the colour pass (advanced indexing for the gathers), checked for the
same words; with --variant_library SO (a `make COLORS=per_slot` build) the entry also holds `mappings`: the colour pass of both
builds on the same tensors, taking turns.  The images here are a function of the pixel and differ from view to view, so the counts say what the kernels did, not
what the rule is worth.  Rows of configurations a call does not run are kept in --out.

    python tools/texture_bench.py [--iters 3] [--views 32,128] [--voxels 0.5,0.25] [--out profiles/texture_bench.json]
        [--smooth_views W [--smooth_max_loss 0.25] [--smooth_rounds 64]] [--outlier_threshold T [--variant_library SO]] [--no_level]
        [--no_local]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_bench as MB  # noqa: E402
from deep3d_aerial_amd import mesh, ortho, texture  # noqa: E402


def ortho_views(mviews):
    """OrthoView records of mesh_bench's views, with an 8-bit image that is a function of the pixel (the fill copies it)."""
    out = []
    for i, v in enumerate(mviews):
        ys, xs = torch.meshgrid(torch.arange(MB.H, device="cuda"), torch.arange(MB.W, device="cuda"), indexing="ij")
        img = torch.stack([(xs + 7 * i) & 255, ys & 255, (xs ^ ys) & 255], -1).to(torch.uint8)
        E = torch.eye(4, dtype=torch.float64).numpy()
        E[:3, :3], E[:3, 3] = v.R, v.t
        out.append(ortho.OrthoView(i, v.K, E, v.depth, img))
    return out


def torch_select(vertices, faces, views, tol=texture.DEFAULT_TOLERANCE):
    """The comparator: texture.py's selection in fp64 torch, one view at a time over every face."""
    V = vertices.double()
    a, b, c = V[faces[:, 0].long()], V[faces[:, 1].long()], V[faces[:, 2].long()]
    e1, e2 = b - a, c - a
    nrm = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    g = ((a + b) + c) / 3.0
    live = (nrm != 0).any(1)
    key = torch.full((faces.shape[0],), texture.EMPTY_KEY, dtype=torch.int64, device=vertices.device)
    for v in views:
        R, t, K, C = v.R.tolist(), v.t.tolist(), v.K.tolist(), v.C.tolist()

        def proj(X):
            p = [R[r][0] * X[:, 0] + R[r][1] * X[:, 1] + R[r][2] * X[:, 2] + t[r] for r in range(3)]
            q = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
            return p[2], q[2], q[0] / q[2], q[1] / q[2]

        ok = live & (nrm[:, 0] * (C[0] - g[:, 0]) + nrm[:, 1] * (C[1] - g[:, 1]) + nrm[:, 2] * (C[2] - g[:, 2]) > 0)
        uv = []
        for X in (a, b, c):
            p2, q2, u, w = proj(X)
            ok &= (p2 > 0) & (q2 > 0) & (u >= 0) & (u <= v.W - 1) & (w >= 0) & (w <= v.H - 1)
            uv.append((u, w))
        p2g, _, ug, vg = proj(g)
        px = torch.floor((ug + 0.5).nan_to_num(0.0).clamp(0, v.W)).clamp(0, v.W - 1).long()
        py = torch.floor((vg + 0.5).nan_to_num(0.0).clamp(0, v.H)).clamp(0, v.H - 1).long()
        D = v.depth.reshape(-1)[py * v.W + px].double()
        ok &= torch.isfinite(D) & (D > 0) & (p2g <= D * (1.0 + tol))
        (ua, va), (ub, vb), (uc, vc) = uv
        A = 0.5 * ((ub - ua) * (vc - va) - (uc - ua) * (vb - va)).abs()
        ok &= A != 0
        s = 1.0 / torch.where(ok, A, torch.ones_like(A))
        ok &= torch.isfinite(s)
        k = (s.float().view(torch.int32).long() << 32) | v.id
        key = torch.where(ok & (k < key), k, key)
    return key


def torch_cg(graph, b, anchor, iterations):
    """The comparator: the solve's iteration in torch on the same CSR (fp32 vectors, fp64 dots, index_add for the row sums), for
    a fixed number of iterations.  Returns x."""
    N = graph.n_nodes
    row = torch.repeat_interleave(torch.arange(N, device=b.device), (graph.row_ptr[1:] - graph.row_ptr[:-1]).long())
    col, w = graph.column.long(), graph.weight[:, None]
    dm = torch.zeros((N, 1), device=b.device).index_add_(0, row, w) + anchor
    x, r = torch.zeros_like(b), b.clone()
    p, q = torch.zeros_like(b), torch.zeros_like(b)
    rr = (r.double() * r.double()).sum(0)
    beta = torch.zeros((4,), device=b.device)
    for _ in range(iterations):
        s = dm * r - torch.zeros_like(r).index_add_(0, row, w * r[col])
        q = s + beta * q
        p = r + beta * p
        alpha = torch.nan_to_num(rr / (p.double() * q.double()).sum(0)).float()
        x = x + alpha * p
        r = r - alpha * q
        t = (r.double() * r.double()).sum(0)
        beta, rr = torch.nan_to_num(t / rr).float(), t
    return x


def level_times(vertices, faces, key, chart, table, packing, ov, atlas, iters):
    """Device-event times of the levelling's passes on the filled atlas (which the apply changes; it is not used afterwards)."""
    out = {}
    n = int(vertices.shape[0])
    t_graph = MB.timed_ms(lambda: out.update(g=texture.level_graph(faces, chart, n)), iters)   # includes torch's sorts and uniques
    graph = out["g"]
    t_samples = MB.timed_ms(lambda: out.update(fb=texture.level_samples(vertices, graph, table, packing, ov, atlas)), iters)
    b = out["fb"][1]
    t_solve = MB.timed_ms(lambda: out.update(s=texture.level_solve(graph, b)), iters)   # includes its state reads and syncs
    g, it, ok = out["s"]
    t_cover = MB.timed_ms(lambda: out.update(c=texture.level_coverage(vertices, faces, chart, table, packing, ov)), iters)
    t_apply = MB.timed_ms(lambda: texture.level_apply(vertices, faces, chart, graph, g, out["c"], table, packing, ov, atlas), iters)
    k = 16
    t_torch = MB.timed_ms(lambda: torch_cg(graph, b, texture.DEFAULT_LEVEL_ANCHOR, k), iters)
    return {"nodes": graph.n_nodes, "seam_pairs": int(graph.seams.shape[0]), "entries": int(graph.column.shape[0]),
            "graph_ms": round(t_graph, 3), "samples_ms": round(t_samples, 3), "solve_ms": round(t_solve, 3), "solve_iterations": it,
            "solve_converged": ok, "solve_ms_per_iteration": round(t_solve / max(it, 1), 4), "coverage_ms": round(t_cover, 3),
            "apply_ms": round(t_apply, 3), "torch_ms_per_iteration": round(t_torch / k, 4)}


def fresh_ms(folded, fn, iters):
    """(the mean device-event time of fn(state) over `iters` calls, the last result): every call, and the warm-up before them, gets
    its own copy of the folded state, made outside the timed region -- the solve works in place, and a solved state is a fixed
    point that the next solve would leave after one sweep."""
    total, res = 0.0, None
    for k in range(iters + 1):
        state = folded.clone()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn(state)
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b) if k else 0.0
    return total / iters, res


def local_times(vertices, faces, chart, table, packing, ov, atlas, iters, radius=texture.DEFAULT_LOCAL_RADIUS,
                iterations=texture.DEFAULT_LOCAL_ITERATIONS):
    """Device-event times of the local levelling's passes on the filled atlas (which the apply changes; it is not used afterwards).
    The band and every solve start from a fresh copy of the folded state.  Beside the whole solve: the charts of the LDS path alone
    and those of the global path alone (the chart table's rows of each), and the LDS path's charts in ONE launch whose workgroups
    all take the LDS of the largest chart, instead of the three launches by LDS class."""
    out = {}
    n = int(vertices.shape[0])
    t_seams = MB.timed_ms(lambda: out.update(s=texture.local_seams(faces, chart, n)), iters)   # includes torch's sort of the pairs
    seams = out["s"]
    t_samples = MB.timed_ms(lambda: out.update(r=texture.local_samples(vertices, seams, table, packing, ov, atlas)), iters)
    texel, rec = out["r"]
    cover = texture.level_coverage(vertices, faces, chart, table, packing, ov)   # the `level` entry times it
    t_fold = MB.timed_ms(lambda: out.update(f=texture.local_fold(texel, rec, cover, packing)), iters)
    del cover
    folded = out["f"]
    solve = lambda tb: (lambda state: texture.local_solve(state, tb, packing, radius, iterations))
    t_band, _ = fresh_ms(folded, lambda state: texture.local_band(state, table, packing, radius), iters)
    t_solve, (state, info) = fresh_ms(folded, solve(table), iters)   # the band and the sweeps, both paths
    classes, _, _ = texture._local_split(table, None)
    in_lds = np.zeros(table.shape[0], bool)
    in_lds[np.concatenate(classes)] = True
    row = {}
    if in_lds.any():
        t, (_, i) = fresh_ms(folded, solve(table[in_lds]), iters)
        row.update({"solve_lds_ms": round(t, 3), "solve_lds_sweeps": i["sweeps"]})
        w, h = table[in_lds, 2].astype(np.int64), table[in_lds, 3].astype(np.int64)
        need = int((((h + 2) * (w + 1) + 4) * texture.LOCAL_WORD_BYTES).max())
        kept, texture.LOCAL_LDS_CLASSES = texture.LOCAL_LDS_CLASSES, (need,)
        try:
            t, _ = fresh_ms(folded, solve(table[in_lds]), iters)
        finally:
            texture.LOCAL_LDS_CLASSES = kept
        row.update({"solve_lds_one_launch_ms": round(t, 3), "one_launch_lds_bytes": need})
    if not in_lds.all():
        t, (_, i) = fresh_ms(folded, solve(table[~in_lds]), iters)
        row.update({"solve_global_ms": round(t, 3), "solve_global_sweeps": i["sweeps"]})
    t_apply = MB.timed_ms(lambda: texture.local_apply(state, table, packing, atlas, radius), iters)
    _, dist, domain, seam = texture.local_fields(state)
    texels = table[:, 2].astype(np.int64) * table[:, 3]
    return dict(row, **{"radius": radius, "iterations": iterations, "seam_edges": int(seams.shape[0]), "records": int(texel.shape[0]),
            "seam_texels": int(seam.sum()), "active_texels": int((domain & (dist >= 1) & (dist <= radius)).sum()),
            "seams_ms": round(t_seams, 3), "samples_ms": round(t_samples, 3), "fold_ms": round(t_fold, 3), "band_ms": round(t_band, 3),
            "solve_ms": round(t_solve, 3), "sweeps": info["sweeps"], "converged": info["converged"], "charts_lds": info["charts_lds"],
            "charts_global": info["charts_global"], "charts_per_lds_class": [int(len(c)) for c in classes],
            "texels_lds_share": round(int(texels[in_lds].sum()) / max(int(texels.sum()), 1), 4), "apply_ms": round(t_apply, 3)})


def smooth_times(vertices, faces, ov, key, before, smooth, iters):
    """The candidates pass, the smoothing and the layout of the smoothed keys, beside `before` (the unsmoothed row's numbers)."""
    weight, max_loss, rounds = smooth
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    out = {}

    def candidates():
        out["cand"] = None   # one list at a time: 128 bytes per face
        out["cand"] = texture.face_candidates(vertices, faces, ov)

    t_cand = MB.timed_ms(candidates, iters)   # includes the fill of the empty list
    cand = out["cand"]
    same = bool(torch.equal(cand[:, 0], key))
    t_smooth = MB.timed_ms(lambda: out.update(s=texture.smooth_views(faces, n, cand, weight, max_loss, rounds)), iters)   # with the incidence
    skey, label, commits = out["s"]
    info = texture.smooth_summary(cand, label, commits, rounds, before["charts"])
    del cand
    out.clear()
    chart, labels = texture.charts(faces, skey, n)
    nc = int(labels.shape[0])
    t_rects = MB.timed_ms(lambda: out.update(r=texture.chart_rects(vertices, faces, skey, chart, nc, ov)), iters)
    rects = out["r"]
    packing = texture.pack(rects)
    table = texture.chart_table(rects, packing, texture.chart_views(skey, labels))
    atlas = texture.new_atlas(packing, "cuda")
    t_fill = MB.timed_ms(lambda: texture.finish_pages(texture.fill_pages(table, packing, ov, atlas.zero_())), iters)
    return {"weight": weight, "max_loss": max_loss, "max_rounds": rounds, "candidates_ms": round(t_cand, 3), "select_ms": before["select_ms"],
            "column_0_is_select": same, "smooth_ms": round(t_smooth, 3), "rounds": info["rounds"], "converged": info["converged"],
            "commits": info["commits"], "charts_before": before["charts"], "charts": nc, "pages_before": before["pages"],
            "pages": packing.n_pages, "atlas_texels_before": before["atlas_texels"], "atlas_texels": int(atlas.numel()),
            "rects_ms_before": before["rects_ms"], "rects_ms": round(t_rects, 3), "fill_ms_before": before["fill_ms"],
            "fill_ms": round(t_fill, 3), "mean_loss": round(info["mean_loss"], 5), "largest_loss": round(info["max_loss"], 5),
            "full_lists": round(info["full_lists"], 4)}


def torch_colors(vertices, faces, cand, views):
    """The comparator: texture.py's colour of a face in a candidate view in fp64 torch, one view at a time over its slots."""
    V = vertices.double()
    col = torch.zeros(cand.shape, dtype=torch.int32, device=cand.device)
    ids = cand & 0xffffffff
    live = cand != texture.EMPTY_KEY
    for v in views:
        f, k = torch.nonzero(live & (ids == v.id), as_tuple=True)
        if not f.numel():
            continue
        R, t, K = v.R.tolist(), v.t.tolist(), v.K.tolist()
        ok = torch.ones_like(f, dtype=torch.bool)
        us, ws = [], []
        for c in range(3):
            X = V[faces[f, c].long()]
            p = [R[r][0] * X[:, 0] + R[r][1] * X[:, 1] + R[r][2] * X[:, 2] + t[r] for r in range(3)]
            q = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
            u, w = q[0] / q[2], q[1] / q[2]
            ok &= (p[2] > 0) & (q[2] > 0) & torch.isfinite(u) & torch.isfinite(w)
            us.append(u)
            ws.append(w)
        mix = lambda p: [((p[0] + p[1]) + p[2]) / 3.0, ((4.0 * p[0] + p[1]) + p[2]) / 6.0, ((4.0 * p[1] + p[0]) + p[2]) / 6.0,
                         ((4.0 * p[2] + p[0]) + p[1]) / 6.0]
        img = v.rgba.reshape(-1, 4)
        total = None
        for su, sw in zip(mix(us), mix(ws)):
            fu, fw = torch.floor(su), torch.floor(sw)
            fx, fy = (su - fu)[:, None], (sw - fw)[:, None]
            x0, y0 = fu.nan_to_num(0.0).clamp(0, v.W - 1).long(), fw.nan_to_num(0.0).clamp(0, v.H - 1).long()
            x1, y1 = (x0 + 1).clamp(max=v.W - 1), (y0 + 1).clamp(max=v.H - 1)
            c = lambda y, x: img[y * v.W + x, :3].double()
            tap = (((1.0 - fx) * (1.0 - fy) * c(y0, x0) + fx * (1.0 - fy) * c(y0, x1)) + (1.0 - fx) * fy * c(y1, x0)) + fx * fy * c(y1, x1)
            total = tap if total is None else total + tap
        q = torch.floor(total + 0.5).nan_to_num(0.0).clamp(0, texture.QUARTER_LEVELS).long()
        word = ((1 << 30) | (q[:, 0] << 20) | (q[:, 1] << 10) | q[:, 2]).int()
        col[f[ok], k[ok]] = word[ok]
    return col


def outlier_times(vertices, faces, ov, threshold, iters, variant=None):
    """The candidates pass, the colour pass and the vote (out of place, so every call sees the same lists), and the torch colour
    pass.  variant: another build of the library (make COLORS=per_slot); its colour pass is then timed on the same tensors, the
    two builds taking turns three times, and checked for the same words."""
    out = {}

    def candidates():
        out["cand"] = None   # one list at a time: 128 bytes per face
        out["cand"] = texture.face_candidates(vertices, faces, ov)

    t_cand = MB.timed_ms(candidates, iters)
    cand = out["cand"]
    col = torch.zeros(cand.shape, dtype=torch.int32, device=cand.device)
    t_col = MB.timed_ms(lambda: texture.face_colors(vertices, faces, cand, ov, col=col), iters)
    spare = torch.empty_like(cand)
    t_vote = MB.timed_ms(lambda: out.update(r=texture.reject_outliers(cand, col, threshold, out=spare)), iters)
    info = texture.outlier_summary(out["r"][2], threshold, cand.shape[0])
    t_torch = MB.timed_ms(lambda: out.update(t=torch_colors(vertices, faces, cand, ov)), iters)
    res = dict(info, candidates_ms=round(t_cand, 3), colors_ms=round(t_col, 3), vote_ms=round(t_vote, 3),
               slots=int((cand != texture.EMPTY_KEY).sum()), coloured_slots=int((col != 0).sum()),
               torch_colors_ms=round(t_torch, 1), torch_same_words=bool(torch.equal(out["t"], col)))
    if variant is not None:
        import ctypes

        other = ctypes.CDLL(variant)
        other.d3d_texture_face_colors.argtypes = texture._lib.SIGNATURES["d3d_texture_face_colors"]
        other.d3d_texture_face_colors.restype = ctypes.c_int
        libs = {"per_face": texture._lib.load(), "per_slot": other}
        P, n, m = texture._ptr, int(vertices.shape[0]), int(faces.shape[0])
        recs, nr = texture._table(ov, vertices.device)
        cols = {k: torch.zeros_like(col) for k in libs}

        def call(k):
            rc = libs[k].d3d_texture_face_colors(P(vertices), n, P(faces), m, P(cand), P(recs), nr, P(cols[k]), texture._stream())
            if rc != 0:
                raise RuntimeError("d3d_texture_face_colors of the %s build: %d" % (k, rc))

        times = {k: [] for k in libs}
        for _ in range(3):
            for k in libs:
                times[k].append(round(MB.timed_ms(lambda: call(k), iters), 3))
        res["mappings"] = {"per_face_ms": times["per_face"], "per_slot_ms": times["per_slot"],
                           "same_words": bool(torch.equal(cols["per_face"], cols["per_slot"]) and torch.equal(cols["per_face"], col))}
    return res


def run(views, voxel, iters, smooth=None, with_level=True, outlier_threshold=None, variant=None, with_local=True):
    grid = mesh.MeshGrid(MB.BORDER, voxel)
    mviews = views
    vertices, faces = mesh.depth_to_mesh(mviews, grid)
    ov = ortho_views(mviews)
    m = int(faces.shape[0])
    n = int(vertices.shape[0])
    lib = texture._lib.load()
    P = texture._ptr
    key = torch.empty((m,), dtype=torch.int64, device="cuda")
    recs, nv = texture._table(ov, "cuda")
    nbytes = int(lib.d3d_texture_scratch_bytes(m, nv))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")

    def select():
        key.fill_(texture.EMPTY_KEY)
        texture._lib.check(lib.d3d_texture_select(P(vertices), n, P(faces), m, P(recs), nv, texture.DEFAULT_TOLERANCE, P(scratch), nbytes,
                                                  P(key), texture._stream()), "select")

    t_select = MB.timed_ms(select, iters)
    out = {}
    t_charts = MB.timed_ms(lambda: out.update(c=texture.charts(faces, key, n)), iters)   # includes its flag reads and one sync
    chart, labels = out["c"]
    nc = int(labels.shape[0])
    t_rects = MB.timed_ms(lambda: out.update(r=texture.chart_rects(vertices, faces, key, chart, nc, ov)), iters)
    rects = out["r"]
    packing = texture.pack(rects)
    table = texture.chart_table(rects, packing, texture.chart_views(key, labels))
    atlas = texture.new_atlas(packing, "cuda")
    t_fill = MB.timed_ms(lambda: texture.finish_pages(texture.fill_pages(table, packing, ov, atlas.zero_())), iters)
    t_tc = MB.timed_ms(lambda: texture.texcoords(vertices, faces, key, chart, table, packing, ov), iters)
    # candidates per face: the views whose tests pass (select over each view alone)
    cand = torch.zeros((m,), dtype=torch.int32, device="cuda")
    for v in ov:
        cand += (texture.select_faces(vertices, faces, [v]) != texture.EMPTY_KEY).int()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tk = torch_select(vertices, faces, ov)
    e1.record()
    torch.cuda.synchronize()
    row = {}
    if with_level:
        texture.fill_pages(table, packing, ov, atlas.zero_())
        row["level"] = level_times(vertices, faces, key, chart, table, packing, ov, atlas, iters)
    if with_local:
        texture.fill_pages(table, packing, ov, atlas.zero_())
        row["local"] = local_times(vertices, faces, chart, table, packing, ov, atlas, iters)
        # the passes of §4.13 in this very run: the only times the column may be set against
        row["local"]["same_run"] = {"select_ms": round(t_select, 3), "charts_ms": round(t_charts, 3), "rects_ms": round(t_rects, 3),
                                    "fill_ms": round(t_fill, 3), "texcoords_ms": round(t_tc, 3)}
    n_texels = int(atlas.numel())
    del atlas, chart, rects, table
    if smooth is not None:
        before = {"charts": nc, "pages": packing.n_pages, "atlas_texels": n_texels, "select_ms": round(t_select, 3),
                  "rects_ms": round(t_rects, 3), "fill_ms": round(t_fill, 3)}
        row["smooth"] = smooth_times(vertices, faces, ov, key, before, smooth, iters)
    if outlier_threshold is not None:
        row["outliers"] = outlier_times(vertices, faces, ov, outlier_threshold, iters, variant)
    return dict(row, **{"views": len(ov), "voxel_m": voxel, "faces": m, "vertices": n, "seen_faces": int((key != texture.EMPTY_KEY).sum()),
            "charts": nc, "pages": packing.n_pages, "atlas_texels": n_texels, "mean_candidates_per_face": round(float(cand.double().mean()), 3),
            "select_ms": round(t_select, 3), "charts_ms": round(t_charts, 3), "rects_ms": round(t_rects, 3), "fill_ms": round(t_fill, 3),
            "texcoords_ms": round(t_tc, 3), "torch_select_ms": round(e0.elapsed_time(e1), 1), "torch_same_keys": bool(torch.equal(tk, key)),
            "face_view_tests": m * len(ov)})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--views", default="32,128")
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.json"))
    ap.add_argument("--smooth_views", type=float, default=None, metavar="W", help="also time the smoothing of the view choice with this weight")
    ap.add_argument("--smooth_max_loss", type=float, default=texture.DEFAULT_SMOOTH_MAX_LOSS)
    ap.add_argument("--smooth_rounds", type=int, default=texture.DEFAULT_SMOOTH_ROUNDS)
    ap.add_argument("--outlier_threshold", type=float, default=None, metavar="T",
                    help="also time the rejection of outlier views with this threshold (0.06 is the reference's fOutlierThreshold)")
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="with --outlier_threshold: a COLORS=per_slot build of the library whose colour pass is timed beside this one")
    ap.add_argument("--no_level", action="store_true", help="skip the seam levelling's times (a row then keeps the recorded `level` entry)")
    ap.add_argument("--no_local", action="store_true", help="skip the local seam levelling's times (a row then keeps the recorded `local` entry)")
    a = ap.parse_args(argv)
    smooth = None
    if a.smooth_views is not None:
        smooth = texture.check_smooth_settings({"weight": a.smooth_views, "max_loss": a.smooth_max_loss, "rounds": a.smooth_rounds})
    if a.outlier_threshold is not None:
        texture.check_outlier_settings({"threshold": a.outlier_threshold})
    if not torch.cuda.is_available():
        raise RuntimeError("tools/texture_bench.py measures the GPU kernels: no GPU here")
    rows = []
    for nv in [int(x) for x in a.views.split(",")]:
        views = MB.make_views(nv, "cuda")
        for voxel in [float(x) for x in a.voxels.split(",")]:
            r = run(views, voxel, a.iters, smooth, not a.no_level, a.outlier_threshold, a.variant_library, not a.no_local)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del views
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "image": [MB.W, MB.H], "border": MB.BORDER, "runs": rows}
    if os.path.exists(a.out):   # rows of other configurations stay, and a row run without an entry keeps the recorded one
        old = json.load(open(a.out))
        done = {(r["views"], r["voxel_m"]): r for r in rows}
        for r in old.get("runs", []):
            mine = done.get((r["views"], r["voxel_m"]))
            if mine is None:
                rows.append(r)
            else:
                for k in ("level", "local", "smooth", "outliers"):
                    if k in r and k not in mine:
                        mine[k] = r[k]
        rows.sort(key=lambda r: (r["views"], -r["voxel_m"]))
        res = dict(old, **res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
