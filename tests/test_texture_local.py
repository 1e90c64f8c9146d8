"""Local seam levelling of the texture on the CPU: a numpy restatement of the rules in deep3d_aerial_amd/texture.py (seam edges,
samples and records, the fold to D, the band, the red-black relaxation and apply; tests/test_texture_local_gpu.py compares the
kernels with it bit for bit) and hand-built cases."""
import os
import re

import numpy as np
import pytest

import test_texture as T
import test_texture_level as L

UNIT = 64      # a correction is an integer in units of 1 / 64 grey level
FAR = 255      # the distance of a texel the band did not reach


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def seams_numpy(faces, chart):
    """[n_seams, 4] (a, b, c1, c2) in increasing (a, b): the edges of exactly two faces (of all faces) that both have a chart,
    in different charts; a < b the ends, c1 < c2 the charts."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    chart = np.asarray(chart, np.int64)
    by_edge = {}
    for f in range(len(F)):
        for e in T.face_edges(F[f]):
            by_edge.setdefault(e, []).append(f)
    out = []
    for (a, b), fs in sorted(by_edge.items()):
        if len(fs) == 2 and chart[fs[0]] >= 0 and chart[fs[1]] >= 0 and chart[fs[0]] != chart[fs[1]]:
            out.append((a, b, min(chart[fs[0]], chart[fs[1]]), max(chart[fs[0]], chart[fs[1]])))
    return np.array(out, np.int32).reshape(-1, 4)


def _rect_of(ch, rects, packing):
    """(ox, row0, w, h) of chart ch in atlas coordinates."""
    x0, y0, x1, y1 = (int(t) for t in rects[ch])
    page, ox, oy = (int(t) for t in packing.place[ch])
    return ox, int(packing.page_row[page]) + oy, x1 - x0 + 1, y1 - y0 + 1


def _vertex_xy(vertices, v, ch, rects, packing, view):
    """The vertex in atlas coordinates of chart ch: X = (u - x0) + ox, Y = ((v - y0) + oy) + page_row, fp64."""
    u, w = L._vertex_uv(view, np.asarray(vertices)[v][None])
    page, ox, oy = (int(t) for t in packing.place[ch])
    return (u[0] - float(rects[ch][0])) + float(ox), ((w[0] - float(rects[ch][1])) + float(oy)) + float(packing.page_row[page])


def tap_numpy(A, box, x, y):
    """The fp64 bilinear tap of A [rows, P, 3] (fp64) at (x, y), the taps kept inside box = (ox, row0, w, h); not rounded."""
    ox, row0, w, h = box
    xf, yf = np.floor(x), np.floor(y)
    tx, ty = x - xf, y - yf
    ix0 = int(min(max(xf, ox), ox + w - 1))
    iy0 = int(min(max(yf, row0), row0 + h - 1))
    ix1, iy1 = min(ix0 + 1, ox + w - 1), min(iy0 + 1, row0 + h - 1)
    w00, w10, w01, w11 = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
    return ((w00 * A[iy0, ix0] + w10 * A[iy0, ix1]) + w01 * A[iy1, ix0]) + w11 * A[iy1, ix1]


def samples_numpy(vertices, seams, rects, packing, chart_ids, views, atlas):
    """{"count" [n_seams] -- S per seam edge --, "texel" [R] int64 and "rec" [R, 3] int32 -- the records in a stable sort by texel
    (row * P + column) of the order (seam edge, sample, chart c1 then c2) --, "diff" [R / 2, 3] fp64 -- colour_c2 - colour_c1 of
    every sample}."""
    by_id = {v["id"]: v for v in views}
    A = np.asarray(atlas)[..., :3].astype(np.float64)
    P = packing.page_size
    count, texel, rec, diff = [], [], [], []
    for a, b, c1, c2 in np.asarray(seams, np.int64):
        ends, boxes = [], []
        for ch in (c1, c2):
            view = by_id[int(chart_ids[ch])]
            ends.append((_vertex_xy(vertices, a, ch, rects, packing, view), _vertex_xy(vertices, b, ch, rects, packing, view)))
            boxes.append(_rect_of(ch, rects, packing))
        Ls = [max(abs(pb[0] - pa[0]), abs(pb[1] - pa[1])) for pa, pb in ends]
        S = int(np.ceil(max(Ls))) + 1
        count.append(S)
        for k in range(S):
            t = k / (S - 1) if S > 1 else 0.0
            col, tex = [], []
            for (pa, pb), box in zip(ends, boxes):
                x, y = pa[0] + t * (pb[0] - pa[0]), pa[1] + t * (pb[1] - pa[1])
                col.append(tap_numpy(A, box, x, y))
                tx = int(min(max(np.floor(x + 0.5), box[0]), box[0] + box[2] - 1))
                ty = int(min(max(np.floor(y + 0.5), box[1]), box[1] + box[3] - 1))
                tex.append(ty * P + tx)
            e = np.floor(32.0 * (col[1] - col[0]) + 0.5).astype(np.int32)
            diff.append(col[1] - col[0])
            texel += tex
            rec += [e, -e]
    texel, rec = np.array(texel, np.int64), np.array(rec, np.int32).reshape(-1, 3)
    order = np.argsort(texel, kind="stable")
    return {"count": np.array(count, np.int32), "texel": texel[order], "rec": rec[order], "diff": np.array(diff, np.float64).reshape(-1, 3)}


def fold_numpy(texel, rec, cover):
    """The state as fields: {"c" [rows, P, 3] int64 -- D on seam texels, 0 elsewhere --, "dist" [rows, P] (0 on seam texels, 255
    elsewhere), "domain", "seam" [rows, P] bool}."""
    domain = np.asarray(cover) != L.EMPTY
    rows, P = domain.shape
    c = np.zeros((rows, P, 3), np.int64)
    seam = np.zeros((rows, P), bool)
    for t in np.unique(texel):
        on = texel == t
        s, n = rec[on].astype(np.int64).sum(0), int(on.sum())
        assert domain[t // P, t % P], "a sample's texel lies within d2 <= 0.5 of a face of its chart: it is covered"
        c[t // P, t % P] = (2 * s + n) // (2 * n)
        seam[t // P, t % P] = True
    return {"c": c, "dist": np.where(seam, 0, FAR).astype(np.uint8), "domain": domain, "seam": seam}


def _neighbours(a, fill):
    """The four 4-neighbours of every entry of a [h, w, ...], `fill` past the border."""
    p = np.full((a.shape[0] + 2, a.shape[1] + 2) + a.shape[2:], fill, a.dtype)
    p[1:-1, 1:-1] = a
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def band_numpy(st, boxes, radius):
    """The breadth-first distance over 4-neighbours inside each rect's domain, from its seam texels; in place."""
    for ox, row0, w, h in boxes:
        sl = (slice(row0, row0 + h), slice(ox, ox + w))
        dom, dist = st["domain"][sl], np.where(st["seam"][sl], 0, FAR).astype(np.int64)
        for r in range(1, radius + 1):
            near = np.zeros(dist.shape, bool)
            for nd, nm in zip(_neighbours(dist, FAR), _neighbours(dom, False)):
                near |= nm & (nd == r - 1)
            new = dom & (dist == FAR) & near
            if not new.any():
                break
            dist[new] = r
        st["dist"][sl] = dist
    return st


def solve_numpy(st, boxes, radius, iterations, snapshots=()):
    """The red-black relaxation per rect, in place.  Returns (sweeps -- those that changed something, the largest over the rects --,
    {k: c after k sweeps for k in snapshots})."""
    per_chart = []
    snaps = {k: st["c"].copy() for k in snapshots}
    for ox, row0, w, h in boxes:
        sl = (slice(row0, row0 + h), slice(ox, ox + w))
        dom, dist, c = st["domain"][sl], st["dist"][sl].astype(np.int64), st["c"][sl].copy()
        active = dom & (dist >= 1) & (dist <= radius)
        ys, xs = np.mgrid[row0:row0 + h, ox:ox + w]
        odd = ((xs + ys) & 1).astype(bool)
        nmask = _neighbours(dom, False)
        n = sum(m.astype(np.int64) for m in nmask)
        run = 0
        for it in range(iterations):
            changed = False
            for parity in (False, True):
                on = active & (odd == parity) & (n > 0)
                s = sum(np.where(m[..., None], v, 0) for v, m in zip(_neighbours(c, 0), nmask))
                new = (2 * s[on] + n[on][:, None]) // (2 * n[on][:, None])
                changed = changed or bool((new != c[on]).any())
                c[on] = new
            if changed:
                run = it + 1
            for k in snapshots:
                if it + 1 <= k:
                    snaps[k][sl] = c
            if not changed:
                break
        st["c"][sl] = c
        per_chart.append(run)
    return max(per_chart) if per_chart else 0, snaps


def apply_numpy(st, atlas, radius):
    """The levelled atlas [rows, P, 3] uint8: every domain texel with dist <= radius moves by (c + 32) >> 6."""
    on = st["domain"] & (st["dist"] <= radius)
    out = np.asarray(atlas).copy()
    out[on] = np.clip(out[on].astype(np.int64) + ((st["c"][on] + 32) >> 6), 0, 255).astype(np.uint8)
    return out


def seam_step(diff):
    """The mean absolute colour step over all seam samples and channels, in grey levels."""
    return float(np.abs(diff).mean()) if len(diff) else 0.0


def local_numpy(vertices, faces, lay, views, atlas, radius=16, iterations=512, snapshots=()):
    """The whole chain on `atlas` [rows, P, 3] with the layout of test_texture_level.level_numpy's result `lay` ("chart", "rects",
    "packing", "ids", "cover"): {"seams", "samples", "D", "state" (after the solve), "sweeps", "snaps", "levelled"}."""
    rects, packing, ids = lay["rects"], lay["packing"], lay["ids"]
    seams = seams_numpy(faces, lay["chart"])
    smp = samples_numpy(vertices, seams, rects, packing, ids, views, atlas)
    st = fold_numpy(smp["texel"], smp["rec"], lay["cover"])
    D = st["c"].copy()
    boxes = [_rect_of(ch, rects, packing) for ch in range(len(rects))]
    band_numpy(st, boxes, radius)
    sweeps, snaps = solve_numpy(st, boxes, radius, iterations, snapshots)
    return {"seams": seams, "samples": smp, "D": D, "state": st, "sweeps": sweeps, "snaps": snaps, "boxes": boxes,
            "levelled": apply_numpy(st, atlas, radius)}


def _hand(V, F, key, vs, page_size=64, pad=2, **kw):
    """The layout, pages and coverage of a hand-built case, and the local levelling on its pages."""
    chart, labels, rects, packing, ids = L.layout_numpy(V, F, key, vs, page_size, pad)
    atlas = L.stack_pages(T.atlas_numpy(rects, packing, ids, vs))
    lay = {"chart": chart, "labels": labels, "rects": rects, "packing": packing, "ids": ids, "atlas": atlas,
           "cover": L.coverage_numpy(V, F, chart, rects, packing, ids, vs)}
    return lay, local_numpy(V, F, lay, vs, atlas, **kw)


# ----------------------------------------------------------------------------------------
# hand-built cases
# ----------------------------------------------------------------------------------------
def test_two_triangles_across_one_seam_meet_in_the_middle():
    """Two flat views of grey 100 and 140: every record is +-32 * 40, so D = +1280 on the dark side and -1280 on the bright side
    and both sides read 120 at the seam; texels past the radius and outside the domain keep their bytes."""
    V = np.array([L._at(20, 20), L._at(20, 30), L._at(8, 25), L._at(32, 25)], np.float32)
    F = np.array([[0, 1, 3], [1, 0, 2]], np.int32)   # the seam is the edge (0, 1): x = 20, y = 20 .. 30
    vs = L._flat_views([(100,) * 3, (140,) * 3])
    key = np.array([T.make_key(1.0, 1), T.make_key(1.0, 2)], np.int64)
    radius = 3
    lay, res = _hand(V, F, key, vs, radius=radius)
    assert res["seams"].tolist() == [[0, 1, 0, 1]] and res["samples"]["count"].tolist() == [11]
    st, P = res["state"], lay["packing"].page_size
    assert st["seam"].sum() == 22
    dark, bright = _rect_of(0, lay["rects"], lay["packing"]), _rect_of(1, lay["rects"], lay["packing"])
    for (ox, row0, w, h), want in ((dark, 1280), (bright, -1280)):
        D = res["D"][row0:row0 + h, ox:ox + w][st["seam"][row0:row0 + h, ox:ox + w]]
        assert len(D) == 11 and (D == want).all()
    assert (res["levelled"][st["seam"]] == 120).all()
    # the correction fades: monotone in the distance on the dark side, and exactly nothing past the radius or outside the domain
    ox, row0, w, h = dark
    row = row0 + h // 2
    first = int(np.flatnonzero(st["seam"][row, ox:ox + w])[0]) + ox   # the face lies to the right of the seam
    along = [int(res["levelled"][row, x, 0]) for x in range(first, ox + w) if st["domain"][row, x]]
    assert along[0] == 120 and sorted(along, reverse=True) == along and along[-1] == 100
    far = st["domain"] & (st["dist"] > radius)
    assert far.any() and (st["dist"][far] == FAR).all() and not st["c"][far].any()
    keep = far | ~st["domain"]
    assert np.array_equal(res["levelled"][keep], lay["atlas"][keep]) and (res["levelled"][~keep] != lay["atlas"][~keep]).any()
    assert (st["dist"][st["domain"] & ~far] <= radius).all() and ((st["dist"] == 0) == st["seam"]).all()


@pytest.mark.parametrize("D", [20 * UNIT, -75 * UNIT + 17, 127 * UNIT + 32])
def test_a_straight_seam_relaxes_to_the_linear_ramp(D):
    """A 40 x 12 chart whose first column is the seam, radius 16, run to the fixed point.  The fixed point lies within one level
    of D (1 - dist / 17) -- the restatement gives 0.53, 0.52 and 0.56 levels for the three D, reached in 161, 267 and 259 sweeps
    -- and is exactly 0 past the radius."""
    h, w, radius = 12, 40, 16
    st = {"c": np.zeros((h, w, 3), np.int64), "domain": np.ones((h, w), bool), "seam": np.zeros((h, w), bool)}
    st["seam"][:, 0] = True
    st["c"][:, 0] = D
    st["dist"] = np.where(st["seam"], 0, FAR).astype(np.uint8)
    band_numpy(st, [(0, 0, w, h)], radius)
    assert np.array_equal(st["dist"][0], np.where(np.arange(w) <= radius, np.arange(w), FAR))
    sweeps, _ = solve_numpy(st, [(0, 0, w, h)], radius, 4000)
    again = {k: v.copy() for k, v in st.items()}
    assert solve_numpy(again, [(0, 0, w, h)], radius, 1)[0] == 0 and 100 < sweeps < 400   # a true fixed point
    dist = st["dist"].astype(np.float64)
    ramp = np.where(dist <= radius, D * (1.0 - dist / (radius + 1)), 0.0)
    off = np.abs(st["c"][..., 0] - ramp).max() / UNIT
    print("D = %d: fixed point after %d sweeps, %.4f levels from the ramp" % (D, sweeps, off))
    assert off <= 1.0
    assert not st["c"][:, radius + 1:].any() and (st["c"][..., 0] == st["c"][..., 2]).all()


def _fan():
    """Three faces around vertex 0 at texel (36, 28), one chart each: F[1] = chart 1 meets chart 0 along (0, 2), chart 2 along (0, 3)."""
    V = np.array([L._at(36, 28), L._at(44, 28), L._at(28, 20), L._at(28, 36)], np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32)
    key = np.array([T.make_key(1.0, k) for k in (1, 2, 3)], np.int64)
    return V, F, key


def test_a_vertex_where_three_charts_meet_averages_the_records_of_both_seams():
    V, F, key = _fan()
    vs = L._flat_views([(100,) * 3, (120,) * 3, (180,) * 3])
    lay, res = _hand(V, F, key, vs, page_size=128)
    assert res["seams"].tolist() == [[0, 1, 0, 2], [0, 2, 0, 1], [0, 3, 1, 2]] and res["samples"]["count"].tolist() == [9, 9, 9]
    ox, row0, w, h = _rect_of(1, lay["rects"], lay["packing"])
    x, y = _vertex_xy(V, 0, 1, lay["rects"], lay["packing"], vs[1])
    t = int(y) * lay["packing"].page_size + int(x)
    assert (x, y) == (int(x), int(y)) and ox <= x < ox + w and row0 <= y < row0 + h
    on = res["samples"]["texel"] == t
    # chart 1 is c2 of its seam with chart 0 (-32 * 20) and c1 of its seam with chart 2 (+32 * 60): D is their mean
    assert sorted(res["samples"]["rec"][on][:, 0].tolist()) == [-640, 1920]
    assert res["D"][int(y), int(x)].tolist() == [640] * 3
    # in charts 0 and 2 the vertex takes both of that chart's seams too
    for ch, want in ((0, (640 + 2560) // 2), (2, -(2560 + 1920) // 2)):
        x, y = _vertex_xy(V, 0, ch, lay["rects"], lay["packing"], vs[ch])
        assert res["D"][int(y), int(x)].tolist() == [want] * 3


def test_a_non_manifold_edge_and_an_edge_next_to_a_face_without_a_winner_give_no_seam_edge():
    assert len(seams_numpy([[0, 1, 2], [1, 0, 3], [0, 1, 4]], [0, 1, 2])) == 0
    assert len(seams_numpy([[0, 1, 2], [1, 0, 3]], [0, -1])) == 0
    assert len(seams_numpy([[0, 1, 2], [1, 0, 3], [0, 1, 4]], [0, 1, -1])) == 0   # three faces on the edge, one without a winner
    assert len(seams_numpy([[0, 1, 2], [1, 0, 3]], [0, 0])) == 0
    assert seams_numpy([[0, 1, 2], [1, 0, 3]], [1, 0]).tolist() == [[0, 1, 0, 1]]   # nothing depends on the face order
    assert seams_numpy(np.zeros((0, 3), np.int32), np.zeros(0, np.int32)).shape == (0, 4)


def test_an_edge_whose_ends_coincide_has_one_sample_and_a_short_one_two():
    """S = ceil(max L) + 1: 1 exactly when the ends coincide in both charts (t = 0), 2 for any shorter-than-a-texel edge, whose
    two samples then share a texel and fold to their mean."""
    vs = L._flat_views([(100,) * 3, (140,) * 3])
    key = np.array([T.make_key(1.0, 1), T.make_key(1.0, 2)], np.int64)
    F = np.array([[0, 1, 3], [1, 0, 2]], np.int32)
    for second, S in ((L._at(20, 20), 1), (L._at(20.25, 20.25), 2)):
        V = np.array([L._at(20, 20), second, L._at(8, 25), L._at(32, 25)], np.float32)
        lay, res = _hand(V, F, key, vs)
        assert res["samples"]["count"].tolist() == [S] and len(res["samples"]["texel"]) == 2 * S
        assert res["state"]["seam"].sum() == 2 and sorted(res["D"][res["state"]["seam"]][:, 0].tolist()) == [-1280, 1280]


def test_one_sweep_and_a_band_of_one_texel():
    V = np.array([L._at(20, 20), L._at(20, 30), L._at(8, 25), L._at(32, 25)], np.float32)
    F = np.array([[0, 1, 3], [1, 0, 2]], np.int32)
    vs = L._flat_views([(100,) * 3, (140,) * 3])
    key = np.array([T.make_key(1.0, 1), T.make_key(1.0, 2)], np.int64)
    lay, one = _hand(V, F, key, vs, radius=8, iterations=1)
    _, full = _hand(V, F, key, vs, radius=8, iterations=512)
    assert one["sweeps"] == 1 and 1 < full["sweeps"] < 512
    # one sweep reaches the texels next to the seam (even ones first, the odd ones see their new values) and no further than 2
    moved = (one["state"]["c"] != one["D"]).any(-1)
    assert moved.any() and (one["state"]["dist"][moved] <= 2).all() and not np.array_equal(one["state"]["c"], full["state"]["c"])
    _, band = _hand(V, F, key, vs, radius=1, iterations=512)
    st = band["state"]
    assert set(np.unique(st["dist"]).tolist()) == {0, 1, FAR} and not st["c"][st["dist"] == FAR].any()
    changed = (band["levelled"] != lay["atlas"]).any(-1)
    assert changed.any() and (st["dist"][changed] <= 1).all()


def test_one_chart_only_leaves_the_pages_as_they_are():
    V, F = T.strip(4)
    vs = L._flat_views([(90, 120, 30)])
    key = np.full(len(F), T.make_key(1.0, 1), np.int64)
    lay, res = _hand(V, F, key, vs)
    assert len(lay["labels"]) == 1 and len(res["seams"]) == 0 and res["sweeps"] == 0
    assert lay["cover"].min() != L.EMPTY and np.array_equal(res["levelled"], lay["atlas"])


def test_argument_errors_of_the_local_settings():
    from deep3d_aerial_amd import texture

    base = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in (["--level_local_radius", "0"], ["--level_local_radius", "255"], ["--level_local_iterations", "0"],
                ["--level_local_iterations", "65536"]):
        for flags in (bad, ["--level_local"] + bad):
            with pytest.raises(SystemExit):
                texture.main(base + flags)
    assert texture.check_local_settings({}) == (16, 512)
    assert texture.check_local_settings({"radius": 254, "iterations": 65535}) == (254, 65535)
    for bad in ({"radius": 0}, {"radius": 255}, {"radius": 2.5}, {"iterations": 0}, {"iterations": 65536}, {"iterations": 1.5},
                {"smooth": 0.1}):
        with pytest.raises(ValueError):
            texture.check_local_settings(bad)


def test_predict_turns_texture_level_local_flags_into_the_stages_settings():
    from deep3d_aerial_amd import predict

    base = ["--output_folder", "out", "--synthetic_items", "2", "--random_weights", "--fuse", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1",
            "--mesh_voxel=0.5", "--texture", "t.ply"]
    s = predict._texture_settings(predict.parse_args(base))
    assert s["local"] is None and s["level"] is None
    a = predict.parse_args(base + ["--texture_level_local", "--texture_level_local_radius", "8"])
    s = predict._texture_settings(a)
    assert s["local"] == {"radius": 8, "iterations": 512} and s["level"] is None
    a = predict.parse_args(base + ["--texture_level", "--texture_level_local", "--texture_level_local_iterations", "40"])
    s = predict._texture_settings(a)
    assert s["local"] == {"radius": 16, "iterations": 40} and s["level"] is not None
    for bad in (["--texture_level_local_radius", "0"], ["--texture_level_local", "--texture_level_local_iterations", "70000"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)


def test_the_header_and_the_binding_carry_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    names = [n for n in _lib.SIGNATURES if n.startswith("d3d_texture_local_")]
    assert sorted(names) == ["d3d_texture_local_" + n for n in ("apply", "band", "chart", "count", "fold", "lds_words", "samples", "seams",
                                                                "sweeps")]
    for n in names:
        assert re.search(r"\b%s\(" % n, text), n
    assert "texture_local.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert os.path.exists(os.path.join(_lib.CSRC, "texture_local.hip"))
