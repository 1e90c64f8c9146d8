"""Mesh texturing on the CPU: a numpy restatement of the semantics in deep3d_aerial_amd/texture.py (select, charts, rects, atlas
and texcoords; tests/test_texture_gpu.py compares the kernels with it bit for bit), checked on hand-built cases; the packing's
invariants; the textured PLY writer and reader."""
import os

import numpy as np
import pytest

EMPTY = np.int64((1 << 63) - 1)
EMPTY_COLOR = (166, 166, 166)


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def make_key(s, vid):
    """(bits(fp32(s)) << 32) | id."""
    return (np.asarray(np.float32(s)).view(np.uint32).astype(np.int64) << 32) | np.int64(vid)


def _cam(v):
    K, E = np.asarray(v["K"], np.float64), np.asarray(v["E"], np.float64)
    R, t = E[:3, :3], E[:3, 3]
    C = np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)])
    return K, R, t, C


def project(v, X):
    """(p2, q2, u, v) of points X [..., 3] fp64 in view v: ortho's projection, rows summed left to right."""
    K, R, t, _ = _cam(v)
    X0, X1, X2 = X[..., 0], X[..., 1], X[..., 2]
    p = [R[r, 0] * X0 + R[r, 1] * X1 + R[r, 2] * X2 + t[r] for r in range(3)]
    q = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
    with np.errstate(all="ignore"):
        return p[2], q[2], q[0] / q[2], q[1] / q[2]


def corners(vertices, faces):
    V = np.asarray(vertices, np.float32).astype(np.float64)
    F = np.asarray(faces, np.int64)
    return V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]


def geometry(vertices, faces):
    a, b, c = corners(vertices, faces)
    e1, e2 = b - a, c - a
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                    e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    g = ((a + b) + c) / 3.0
    return a, b, c, nrm, g


def select_numpy(vertices, faces, views, depth_tolerance=0.01):
    """key [m] int64: the smallest (bits(fp32(1 / A)) << 32) | id over the candidate views of each face."""
    a, b, c, nrm, g = geometry(vertices, faces)
    m = a.shape[0]
    key = np.full(m, EMPTY, np.int64)
    live = (nrm != 0).any(1)
    for v in views:
        _, _, _, C = _cam(v)
        H, W = v["depth"].shape
        ok = live & (nrm[:, 0] * (C[0] - g[:, 0]) + nrm[:, 1] * (C[1] - g[:, 1]) + nrm[:, 2] * (C[2] - g[:, 2]) > 0)
        uv = []
        for X in (a, b, c):
            p2, q2, u, w = project(v, X)
            with np.errstate(invalid="ignore"):
                ok &= (p2 > 0) & (q2 > 0) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
            uv.append((u, w))
        p2g, _, ug, vg = project(v, g)
        with np.errstate(invalid="ignore"):
            px = np.clip(np.floor(np.clip(np.nan_to_num(ug + 0.5), 0, W)), 0, W - 1).astype(np.int64)
            py = np.clip(np.floor(np.clip(np.nan_to_num(vg + 0.5), 0, H)), 0, H - 1).astype(np.int64)
            D = v["depth"][py, px].astype(np.float64)
            ok &= np.isfinite(D) & (D > 0) & (p2g <= D * (1.0 + depth_tolerance))
            (ua, va), (ub, vb), (uc, vc) = uv
            A = 0.5 * np.abs((ub - ua) * (vc - va) - (uc - ua) * (vb - va))
            ok &= A != 0
            s = 1.0 / np.where(ok, A, 1.0)
            ok &= np.isfinite(s)
        k = make_key(s, v["id"])
        key = np.where(ok & (k < key), k, key)
    return key


def face_edges(f):
    a, b, c = (int(x) for x in f)
    out = []
    for x, y in ((a, b), (b, c), (c, a)):
        if x != y and (min(x, y), max(x, y)) not in out:
            out.append((min(x, y), max(x, y)))
    return out


def charts_numpy(faces, key):
    """(chart [m] int32, -1 without a winner; labels [n_charts]): faces joined across shared edges with the same winning id."""
    m = len(faces)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    owner = {}
    for f in range(m):
        if key[f] == EMPTY:
            continue
        wid = int(key[f] & 0xffffffff)
        for e in face_edges(faces[f]):
            o = owner.setdefault((e, wid), f)
            ra, rb = find(o), find(f)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(f) for f in range(m)], np.int64)
    live = key != EMPTY
    labels = np.flatnonzero(live & (roots == np.arange(m)))
    number = np.full(m, -1, np.int64)
    number[labels] = np.arange(len(labels))
    chart = np.where(live, number[roots], -1).astype(np.int32)
    return chart, labels


def rects_numpy(vertices, faces, key, chart, n_charts, views, pad=2):
    by_id = {v["id"]: v for v in views}
    a, b, c = corners(vertices, faces)
    rect = np.zeros((n_charts, 4), np.int64)
    for ch in range(n_charts):
        fs = np.flatnonzero(chart == ch)
        v = by_id[int(key[fs[0]] & 0xffffffff)]
        H, W = v["depth"].shape
        us, vs = [], []
        for X in (a[fs], b[fs], c[fs]):
            _, _, u, w = project(v, X)
            us.append(u)
            vs.append(w)
        us, vs = np.concatenate(us), np.concatenate(vs)
        rect[ch] = (max(0, np.floor(us.min()) - pad), max(0, np.floor(vs.min()) - pad), min(W - 1, np.ceil(us.max()) + pad),
                    min(H - 1, np.ceil(vs.max()) + pad))
    return rect.astype(np.int32)


def atlas_numpy(rects, packing, chart_ids, views, empty=EMPTY_COLOR):
    by_id = {v["id"]: v for v in views}
    pages = [np.empty((h, packing.page_size, 3), np.uint8) for h in packing.heights]
    for p in pages:
        p[...] = empty
    for ch, (x0, y0, x1, y1) in enumerate(np.asarray(rects, np.int64)):
        k, ox, oy = packing.place[ch]
        img = by_id[int(chart_ids[ch])]["image"]
        pages[k][oy:oy + y1 - y0 + 1, ox:ox + x1 - x0 + 1] = img[y0:y1 + 1, x0:x1 + 1, :3]
    return pages


def texcoords_numpy(vertices, faces, key, chart, rects, packing, views):
    by_id = {v["id"]: v for v in views}
    a, b, c = corners(vertices, faces)
    m = a.shape[0]
    P = float(packing.page_size)
    tc = np.empty((m, 6), np.float32)
    tc[:, 0::2] = np.float32(1.0 / P)
    tc[:, 1::2] = np.float32(1.0 - 1.0 / packing.heights[0])
    tn = np.zeros(m, np.int32)
    for f in np.flatnonzero(chart >= 0):
        ch = chart[f]
        v = by_id[int(key[f] & 0xffffffff)]
        x0, y0 = float(rects[ch][0]), float(rects[ch][1])
        k, ox, oy = (int(x) for x in packing.place[ch])
        hp = float(packing.heights[k])
        for q, X in enumerate((a[f], b[f], c[f])):
            _, _, u, w = project(v, X[None])
            tc[f, 2 * q] = np.float32((((u[0] - x0) + ox) + 0.5) / P)
            tc[f, 2 * q + 1] = np.float32(1.0 - (((w[0] - y0) + oy) + 0.5) / hp)
        tn[f] = k
    return tc, tn


def texture_numpy(vertices, faces, views, depth_tolerance=0.01, page_size=8192, pad=2):
    """The whole chain; the packing is texture.pack's (host code)."""
    from deep3d_aerial_amd import texture

    key = select_numpy(vertices, faces, views, depth_tolerance)
    chart, labels = charts_numpy(faces, key)
    rects = rects_numpy(vertices, faces, key, chart, len(labels), views, pad)
    packing = texture.pack(rects, page_size)
    ids = (key[labels] & 0xffffffff).astype(np.int64)
    pages = atlas_numpy(rects, packing, ids, views)
    tc, tn = texcoords_numpy(vertices, faces, key, chart, rects, packing, views)
    return {"key": key, "chart": chart, "labels": labels, "rects": rects, "packing": packing, "pages": pages, "texcoord": tc,
            "texnumber": tn}


# ----------------------------------------------------------------------------------------
# hand-built cases
# ----------------------------------------------------------------------------------------
def cam_view(vid, C=(0.0, 0.0, 0.0), w=64, h=48, f=40.0, depth=10.0):
    """A camera at C looking along +Z (x right, y down), depth map constant `depth`, image a ramp."""
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = -np.asarray(C, np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    img = np.stack([xs * 3 % 256, ys * 5 % 256, (xs + ys) % 256], -1).astype(np.uint8)
    return {"id": vid, "K": K, "E": E, "depth": np.full((h, w), depth, np.float32), "image": img}


# a face on z = 10 whose normal points at the cameras (-Z)
TRI = np.array([[0.0, 0.0, 10.0], [0.0, 1.0, 10.0], [1.0, 0.0, 10.0]], np.float32)


def test_a_front_facing_face_takes_the_view_and_a_back_facing_one_does_not():
    v = cam_view(7)
    key = select_numpy(TRI, [[0, 1, 2], [0, 2, 1]], [v])
    assert key[1] == EMPTY and key[0] != EMPTY
    assert int(key[0] & 0xffffffff) == 7
    # the key is 1 / the projected area: a right triangle of legs f * 1 / 10 = 4 px
    assert key[0] == make_key(1.0 / 8.0, 7)


def test_a_face_half_off_the_image_takes_the_view_that_sees_it_whole():
    tri = TRI + np.float32([-8.5, 0.0, 0.0])   # x from -8.5 to -7.5
    near = cam_view(1, f=40.0)   # u = 31.5 + 4 x: -2.5 .. 1.5, one corner off the image
    far = cam_view(2, f=10.0)    # u = 31.5 + x: 23 .. 24, inside, smaller
    key = select_numpy(tri, [[0, 1, 2]], [near, far])
    assert int(key[0] & 0xffffffff) == 2
    assert select_numpy(tri, [[0, 1, 2]], [near])[0] == EMPTY


def test_an_occluded_face_takes_the_view_that_sees_it():
    hidden = cam_view(1, depth=9.0)   # the surface this view saw lies 1 m in front of the face
    seen = cam_view(2, f=20.0)
    key = select_numpy(TRI, [[0, 1, 2]], [hidden, seen])
    assert int(key[0] & 0xffffffff) == 2
    # within the tolerance the face is not hidden: 10 <= 9.95 * 1.01
    assert int(select_numpy(TRI, [[0, 1, 2]], [cam_view(1, depth=9.95), seen])[0] & 0xffffffff) == 1
    # holes in depth (0, NaN) take nothing
    for d in (0.0, np.nan):
        assert select_numpy(TRI, [[0, 1, 2]], [cam_view(1, depth=d)])[0] == EMPTY


def test_a_degenerate_face_gets_no_view():
    pts = np.array([[0.0, 0.0, 10.0], [1.0, 1.0, 10.0], [2.0, 2.0, 10.0]], np.float32)
    key = select_numpy(pts, [[0, 1, 2], [0, 0, 1]], [cam_view(1)])
    assert (key == EMPTY).all()


def test_an_exact_tie_goes_to_the_lower_id_whatever_the_order():
    a, b = cam_view(9), cam_view(4)
    for vs in ([a, b], [b, a]):
        key = select_numpy(TRI, [[0, 1, 2]], vs)
        assert int(key[0] & 0xffffffff) == 4


def strip(n=6):
    """A strip of 2 n triangles on z = 10, x in 0 .. n, y in 0 .. 1, every normal toward -Z."""
    xs = np.arange(n + 1, dtype=np.float32)
    V = np.concatenate([np.stack([xs, np.zeros_like(xs), np.full_like(xs, 10)], 1), np.stack([xs, np.ones_like(xs), np.full_like(xs, 10)], 1)])
    F = []
    for i in range(n):
        lo0, lo1, hi0, hi1 = i, i + 1, n + 1 + i, n + 2 + i
        F += [[lo0, hi0, lo1], [lo1, hi0, hi1]]
    return V.astype(np.float32), np.array(F, np.int32)


def test_charts_join_faces_across_edges_with_the_same_winner_and_number_them_by_label():
    V, F = strip(6)
    key = np.full(len(F), EMPTY, np.int64)
    key[:4] = make_key(1.0, 3)
    key[4:8] = make_key(2.0, 5)
    key[9:] = make_key(0.5, 3)    # face 8 has no winner: it cuts the view-3 faces in two charts
    chart, labels = charts_numpy(F, key)
    assert list(labels) == [0, 4, 9]
    assert list(chart) == [0, 0, 0, 0, 1, 1, 1, 1, -1, 2, 2, 2]
    # a shared vertex is not enough: faces 0 and 2 share vertex 1 only through face 1
    key2 = key.copy()
    key2[1] = make_key(1.0, 5)
    chart2, labels2 = charts_numpy(F, key2)
    assert chart2[0] != chart2[2]


def test_rects_pad_and_clamp_to_the_image():
    v = cam_view(1, f=40.0)
    V, F = strip(2)
    key = select_numpy(V, F, [v])
    chart, labels = charts_numpy(F, key)
    assert len(labels) == 1
    rect = rects_numpy(V, F, key, chart, 1, [v], pad=2)
    # u = 31.5 + 4 x for x in 0 .. 2, v = 23.5 + 4 y for y in 0 .. 1
    assert list(rect[0]) == [31 - 2, 23 - 2, 40 + 2, 28 + 2]
    rect = rects_numpy(V, F, key, chart, 1, [v], pad=40)
    assert list(rect[0]) == [0, 0, 63, 47]


def test_atlas_and_texcoords_of_one_chart():
    from deep3d_aerial_amd import texture

    v = cam_view(1, f=40.0)
    V, F = strip(2)
    res = texture_numpy(V, F, [v], page_size=64)
    (x0, y0, x1, y1), = res["rects"]
    k, ox, oy = res["packing"].place[0]
    assert (k, ox, oy) == (0, 2, 0) and res["packing"].heights == [y1 - y0 + 1]
    page = res["pages"][0]
    assert (page[oy:oy + y1 - y0 + 1, ox:ox + x1 - x0 + 1] == v["image"][y0:y1 + 1, x0:x1 + 1]).all()
    assert (page[:2, :2] == EMPTY_COLOR).all() and (page[:, ox + x1 - x0 + 1:] == EMPTY_COLOR).all()
    # the texcoord of a corner maps back to its pixel: s P - 0.5 = u - x0 + ox
    _, _, u, w = project(v, V[F[0]].astype(np.float64))
    assert np.allclose(res["texcoord"][0, 0::2] * 64 - 0.5, u - x0 + ox, atol=1e-4)
    assert np.allclose((1 - res["texcoord"][0, 1::2]) * page.shape[0] - 0.5, w - y0 + oy, atol=1e-4)
    assert texture.EMPTY_COLOR == EMPTY_COLOR


def test_a_face_without_a_winner_points_at_the_empty_block():
    V, F = strip(2)
    res = texture_numpy(V, F, [cam_view(1, C=(100.0, 0.0, 0.0))], page_size=64)
    assert (res["key"] == EMPTY).all() and len(res["labels"]) == 0
    assert res["packing"].heights == [2]
    assert (res["pages"][0] == EMPTY_COLOR).all()
    assert np.array_equal(res["texcoord"][0], np.float32([1 / 64, 0.5] * 3)) and (res["texnumber"] == 0).all()


# ----------------------------------------------------------------------------------------
# packing
# ----------------------------------------------------------------------------------------
def _random_rects(rng, n, W=300, H=200):
    x0 = rng.integers(0, W - 1, n)
    y0 = rng.integers(0, H - 1, n)
    x1 = np.minimum(x0 + rng.integers(1, 60, n), W - 1)
    y1 = np.minimum(y0 + rng.integers(1, 40, n), H - 1)
    return np.stack([x0, y0, x1, y1], 1).astype(np.int32)


@pytest.mark.parametrize("seed,n,P", [(0, 1, 300), (1, 50, 300), (2, 800, 300), (3, 3000, 512)])
def test_packing_invariants(seed, n, P):
    from deep3d_aerial_amd import texture

    rects = _random_rects(np.random.default_rng(seed), n)
    pk = texture.pack(rects, P)
    w, h = rects[:, 2] - rects[:, 0] + 1, rects[:, 3] - rects[:, 1] + 1
    page, ox, oy = pk.place[:, 0], pk.place[:, 1], pk.place[:, 2]
    assert pk.page_size == P and pk.n_pages == page.max() + 1
    assert (ox >= 0).all() and (oy >= 0).all() and (ox + w <= P).all()
    assert (oy + h <= np.array(pk.heights)[page]).all() and max(pk.heights) <= P
    for k in range(pk.n_pages):   # no two rects overlap, and none covers page 0's empty block
        cover = np.zeros((pk.heights[k], P), np.int32)
        if k == 0:
            cover[:2, :2] += 1
        for i in np.flatnonzero(page == k):
            cover[oy[i]:oy[i] + h[i], ox[i]:ox[i] + w[i]] += 1
        assert cover.max() == 1
        assert pk.heights[k] == max(oy[page == k] + h[page == k]) if (page == k).any() else pk.heights[k] == 2
    # the order: (height desc, width desc, label asc) runs through the pages, top to bottom, left to right
    order = np.lexsort((np.arange(n), -w, -h))
    pos = np.lexsort((ox[order], oy[order], page[order]))
    assert (pos == np.arange(n)).all()
    # deterministic
    again = texture.pack(rects, P)
    assert np.array_equal(again.place, pk.place) and again.heights == pk.heights


def test_pack_refuses_rects_wider_than_a_page():
    from deep3d_aerial_amd import texture

    with pytest.raises(ValueError):
        texture.pack(np.array([[0, 0, 10, 3]], np.int32), 8)
    with pytest.raises(ValueError):
        texture.check_pad(0)
    assert texture.pack(np.zeros((0, 4), np.int32), 16).heights == [2]


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def test_write_and_read_the_textured_ply(tmp_path):
    from PIL import Image

    from deep3d_aerial_amd import texture

    rng = np.random.default_rng(5)
    V = rng.standard_normal((7, 3)).astype(np.float32)
    F = rng.integers(0, 7, (5, 3)).astype(np.int32)
    tc = rng.uniform(0, 1, (5, 6)).astype(np.float32)
    tn = np.array([0, 1, 1, 0, 1], np.int32)
    pages = [rng.integers(0, 256, (4, 8, 3)).astype(np.uint8), rng.integers(0, 256, (3, 8, 3)).astype(np.uint8)]
    paths = texture.write_textured_ply(str(tmp_path / "m.ply"), V, F, tc, tn, pages)
    assert [os.path.basename(p) for p in paths] == ["m.ply", "m_0.png", "m_1.png"]
    data = (tmp_path / "m.ply").read_bytes()
    header = (b"ply\nformat binary_little_endian 1.0\ncomment TextureFile m_0.png\ncomment TextureFile m_1.png\nelement vertex 7\n"
              b"property float x\nproperty float y\nproperty float z\nelement face 5\nproperty list uchar int vertex_indices\n"
              b"property list uchar float texcoord\nproperty int texnumber\nend_header\n")
    assert data[:len(header)] == header and len(data) == len(header) + 7 * 12 + 5 * 42
    face0 = data[len(header) + 84:len(header) + 84 + 42]
    assert face0[0] == 3 and face0[13] == 6 and np.frombuffer(face0[14:38], "<f4").tolist() == tc[0].tolist()
    v, f, t, k, files = texture.read_textured_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(v, V) and np.array_equal(f, F) and np.array_equal(t, tc) and np.array_equal(k, tn)
    assert files == ["m_0.png", "m_1.png"]
    for p, page in zip(paths[1:], pages):
        im = Image.open(p)
        assert im.mode == "RGB" and np.array_equal(np.array(im), page)


def test_the_untextured_ply_is_unchanged(tmp_path):
    from deep3d_aerial_amd import mesh

    V, F = strip(2)
    mesh.write_ply(str(tmp_path / "a.ply"), V, F)
    assert (tmp_path / "a.ply").read_bytes().startswith(mesh.ply_header(len(V), len(F)))
    assert b"texcoord" not in (tmp_path / "a.ply").read_bytes()


def test_argument_errors(capsys):
    from deep3d_aerial_amd import texture

    for bad in (["--pad", "0"], ["--page_size", "1"], ["--depth_tolerance", "-1"], ["--views_per_batch", "0"]):
        with pytest.raises(SystemExit):
            texture.main(["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"] + bad)
    with pytest.raises(SystemExit):
        texture.main(["--mesh", "m.ply", "--mvs", "x", "--out", "o.obj"])
