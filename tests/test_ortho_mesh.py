"""CPU checks of the orthophoto of the textured mesh (deep3d_aerial_amd/ortho_mesh.py, csrc/ortho_mesh.hip).
`mesh_ortho_numpy` restates the rule of ortho_mesh.py's docstring in numpy: a brute force in fp64 over every (triangle, cell)
pair, on test_dsm_mesh's triangles and cell ranges and with test_ortho's bilinear colour.  It is checked here on analytic
scenes, and tests/test_ortho_mesh_gpu.py compares the kernels against it bit for bit.  Also: the C ABI and its argument checks,
the operator's refusals, the settings, both command lines and the pipeline's up-front validation."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import test_dsm_mesh as T
from deep3d_aerial_amd import _lib, dsm, ortho_mesh, pipeline, predict, texture

NEW_SYMBOLS = ("d3d_ortho_mesh_scratch_bytes", "d3d_ortho_from_mesh")


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def sorted_corners(vertices, faces):
    """(ids [m'] of the faces the rasteriser uses, corner [m',3]: the corner of the face that is vertex k of the lexicographic
    order), in the order test_dsm_mesh.triangles keeps them."""
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.flatnonzero(((F >= 0) & (F < len(V))).all(1))
    P = V[F[ids]].copy()
    fin = np.isfinite(P).all((1, 2))
    ids, P = ids[fin], P[fin]
    C = np.tile(np.arange(3), (len(ids), 1))
    for i, j in ((0, 1), (1, 2), (0, 1)):
        K = T.keys_of(P)
        sw = T._less(K[:, j], K[:, i])
        a, b = P[:, i].copy(), P[:, j].copy()
        P[:, i], P[:, j] = np.where(sw[:, None], b, a), np.where(sw[:, None], a, b)
        ca, cb = C[:, i].copy(), C[:, j].copy()
        C[:, i], C[:, j] = np.where(sw, cb, ca), np.where(sw, ca, cb)
    ox, oy, ex, ey, s = T._edge(P[:, 0], P[:, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        D = s * (ex * (P[:, 2, 1].astype(np.float64) - oy) - ey * (P[:, 2, 0].astype(np.float64) - ox))
    keep = (D != 0) & np.isfinite(D)
    return ids[keep], C[keep]


def atlas_of(pages):
    """pages [[h_k, P, 3 or 4] uint8] -> (rgb [rows, P, 3] uint8, page_row [n_pages + 1])."""
    pages = [np.asarray(p, np.uint8)[:, :, :3] for p in pages]
    return np.concatenate(pages, 0), np.concatenate([[0], np.cumsum([p.shape[0] for p in pages])]).astype(np.int64)


def tap(rgb, row0, P, h, x, y):
    """The bilinear colour of ortho.py (test_ortho.ortho_numpy's, with the lower clamp a texel position needs) on the page of h
    rows starting at row0 of rgb: [n, 3] float64, not rounded."""
    fu, fv = np.floor(x), np.floor(y)
    fx, fy = x - fu, y - fv
    x0 = np.clip(fu, 0, P - 1).astype(np.int64)
    y0 = np.clip(fv, 0, h - 1).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, P - 1), np.minimum(y0 + 1, h - 1)
    w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    out = np.empty((len(x), 3))
    for ch in range(3):
        c = lambda yy, xx: rgb[row0 + yy, xx, ch].astype(np.float64)
        out[:, ch] = w00 * c(y0, x0) + w10 * c(y0, x1) + w01 * c(y1, x0) + w11 * c(y1, x1)
    return out


def untextured(texcoord, texnumber, n_pages):
    tc = np.ascontiguousarray(texcoord, np.float32).reshape(-1, 6)
    b = tc.view(np.uint32)
    same = (b[:, 0] == b[:, 2]) & (b[:, 2] == b[:, 4]) & (b[:, 1] == b[:, 3]) & (b[:, 3] == b[:, 5])
    tn = np.asarray(texnumber, np.int64)
    return same | ~np.isfinite(tc).all(1) | (tn < 0) | (tn >= n_pages)


def mesh_ortho_numpy(vertices, faces, texcoord, texnumber, pages, grid, z_down=False, chunk=1 << 21):
    """(key [H,W] uint64, rgba [H,W,4] uint8, height [H,W] float32) as ortho_mesh.py's docstring states them."""
    edges, z, box = T.triangles(vertices, faces)
    ids, corner = sorted_corners(vertices, faces)
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(ids) == len(z) and np.array_equal(V[F[ids[:, None], corner], 2].astype(np.float64), z)   # the same faces, the same order
    tc = np.ascontiguousarray(texcoord, np.float32).reshape(-1, 6)
    tn = np.asarray(texnumber, np.int64).reshape(-1)
    rgb, page_row = atlas_of(pages)
    n_pages, P = len(page_row) - 1, rgb.shape[1]
    plain = untextured(tc, tn, n_pages)[ids]
    S = np.take_along_axis(tc[ids][:, 0::2], corner, 1).astype(np.float64)   # texcoords of the sorted vertices
    Tt = np.take_along_axis(tc[ids][:, 1::2], corner, 1).astype(np.float64)
    page = np.where(plain, 0, tn[ids])
    j0, j1, i0, i1, ok = T.cell_ranges(box, grid)
    nj, ni = np.where(ok, j1 - j0 + 1, 0), np.where(ok, i1 - i0 + 1, 0)
    n = nj * ni
    key = np.zeros(grid.width * grid.height, np.uint64)
    start = 0
    while start < len(n):
        end, tot = start, 0
        while end < len(n) and (end == start or tot + n[end] <= chunk):
            tot += n[end]
            end += 1
        sl = slice(start, end)
        tri = np.repeat(np.arange(start, end), n[sl])
        local = np.arange(tot) - np.repeat(np.cumsum(n[sl]) - n[sl], n[sl])
        i = i0[tri] + local // np.maximum(nj[tri], 1)
        j = j0[tri] + local % np.maximum(nj[tri], 1)
        px = grid.x_min + (j.astype(np.float64) + 0.5) * grid.unit[0]
        py = grid.y_max - (i.astype(np.float64) + 0.5) * grid.unit[1]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            w = [e[4][tri] * (e[2][tri] * (py - e[1][tri]) - e[3][tri] * (px - e[0][tri])) for e in edges]
            W = (w[0] + w[1]) + w[2]
            cov = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (W > 0)
            Wd = np.where(cov, W, 1.0)
            zz = (((w[0] * z[tri, 0] + w[1] * z[tri, 1]) + w[2] * z[tri, 2]) / Wd).astype(np.float32)
            cov &= (zz.astype(np.float64) >= grid.z_min) & (zz.astype(np.float64) <= grid.z_max)
            s = ((w[0] * S[tri, 0] + w[1] * S[tri, 1]) + w[2] * S[tri, 2]) / Wd
            t = ((w[0] * Tt[tri, 0] + w[1] * Tt[tri, 1]) + w[2] * Tt[tri, 2]) / Wd
        word = np.zeros(tot, np.uint64)
        tex = cov & ~plain[tri]
        for k in np.unique(page[tri][tex]):
            m = np.flatnonzero(tex & (page[tri] == k))
            h = int(page_row[k + 1] - page_row[k])
            x = s[m] * float(P) - 0.5
            y = (1.0 - t[m]) * float(h) - 0.5
            c = np.clip(np.floor(tap(rgb, int(page_row[k]), P, h, x, y) + 0.5), 0, 255).astype(np.uint64)
            word[m] = c[:, 0] | (c[:, 1] << np.uint64(8)) | (c[:, 2] << np.uint64(16)) | np.uint64(0xff000000)
        zk = T.keys_of(zz[cov])
        if z_down:
            zk = ~zk
        np.maximum.at(key, (i * grid.width + j)[cov], (zk.astype(np.uint64) << np.uint64(32)) | word[cov])
        start = end
    zk = (key >> np.uint64(32)).astype(np.uint32)
    height = np.where(key == 0, np.float32(np.nan), T.unkey(~zk if z_down else zk)).astype(np.float32).reshape(grid.shape)
    lo = (key & np.uint64(0xffffffff)).astype("<u4")
    rgba = lo.view(np.uint8).reshape(grid.height, grid.width, 4).copy()
    return key.reshape(grid.shape), rgba, height


# ----------------------------------------------------------------------------------------
# scenes (shared with tests/test_ortho_mesh_gpu.py)
# ----------------------------------------------------------------------------------------
def planar_texcoords(V, F, extent):
    """Texcoords that lay the page over the XY rectangle extent = (x0, x1, y0, y1): texel (x, y) of a P x h page sits at world
    (x0 + (x + 0.5) / P (x1 - x0), y1 - (y + 0.5) / h (y1 - y0)), i.e. s = (X - x0) / (x1 - x0), t = (Y - y0) / (y1 - y0)."""
    x0, x1, y0, y1 = extent
    P3 = np.asarray(V, np.float64)[np.asarray(F, np.int64)]
    tc = np.empty((len(F), 6), np.float32)
    tc[:, 0::2] = (P3[:, :, 0] - x0) / (x1 - x0)
    tc[:, 1::2] = (P3[:, :, 1] - y0) / (y1 - y0)
    return tc


def ramp_page(h, P):
    """R rises by 2 per texel in x, G by 3 per texel in y, B is their sum halved: linear, so a bilinear tap is exact."""
    y, x = np.mgrid[0:h, 0:P]
    return np.stack([20 + 2 * x, 10 + 3 * y, 15 + x + 1.5 * y], -1).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rotate(F, tc, r):
    """Faces with their corners rotated by r, the texcoords along."""
    idx = [(k + r) % 3 for k in range(3)]
    return F[:, idx], tc.reshape(-1, 3, 2)[:, idx].reshape(-1, 6)


def reverse(F, tc):
    return F[:, ::-1], tc.reshape(-1, 3, 2)[:, ::-1].reshape(-1, 6)


# ----------------------------------------------------------------------------------------
def test_a_tilted_quad_with_a_ramp_atlas_gives_back_the_ramp():
    g = dsm.DsmGrid([0.0, 12.0, 0.0, 9.0], [0.25, 0.5])
    ext = (-1.0, 13.0, -2.0, 10.0)
    f = lambda x, y: 0.3 * x - 0.7 * y + 20.0
    V, F = T.quad(ext[0], ext[1], ext[2], ext[3], f)
    P, h = 40, 30
    ramp = ramp_page(h, P)
    assert ramp.max() < 255
    page = np.floor(ramp).astype(np.uint8)
    tc = planar_texcoords(V, F, ext)
    key, rgba, height = mesh_ortho_numpy(V, F, tc, np.zeros(2, np.int32), [page], g)
    assert (rgba[:, :, 3] == 255).all() and not np.isnan(height).any()
    cx = g.x_min + (np.arange(g.width) + 0.5) * g.unit[0]
    cy = g.y_max - (np.arange(g.height) + 0.5) * g.unit[1]
    X, Y = np.meshgrid(cx, cy)
    x = (X - ext[0]) / (ext[1] - ext[0]) * P - 0.5         # the texel position of the centre
    y = (1 - (Y - ext[2]) / (ext[3] - ext[2])) * h - 0.5
    # R and G are exact ramps of integers: the tap returns them up to the rounding of s, t (fp32 texcoords: 2^-24 of P texels)
    want = np.stack([20 + 2 * x, 10 + 3 * y], -1)
    got = rgba[:, :, :2].astype(np.float64)
    assert (np.abs(got - want) <= 0.5 + 1e-3).all(), np.abs(got - want).max()
    # B holds floor(15 + x + 1.5 y): the ramp to within the floor of the texels
    wantb = 15 + x + 1.5 * y
    assert (np.abs(rgba[:, :, 2] - wantb) <= 1.0 + 1e-3).all()
    assert (np.abs(height - f(X, Y).astype(np.float32)) <= 2 * np.spacing(np.abs(f(X, Y)).astype(np.float32))).all()


def _field(seed, n=14):
    V, F = T.height_field(n, seed, spacing=1.1, origin=0.3)
    rng = np.random.default_rng(seed + 50)
    tc = rng.uniform(0.02, 0.98, (len(F), 6)).astype(np.float32)
    tn = rng.integers(0, 2, len(F)).astype(np.int32)
    pages = [rng.integers(0, 256, (h, 32, 3), dtype=np.uint8) for h in (20, 13)]
    return V, F, tc, tn, pages


def test_height_is_the_mesh_dsm_and_z_down_is_the_mirrored_mesh_negated():
    g = T.grid_small()
    for V, F in (T.height_field(16, 3, spacing=1.1, origin=0.3), T.soup(300, 4), T.box_building()):
        rng = np.random.default_rng(1)
        tc = rng.uniform(0, 1, (len(F), 6)).astype(np.float32)
        tn = np.zeros(len(F), np.int32)
        pages = [rng.integers(0, 256, (9, 16, 3), dtype=np.uint8)]
        _, _, up = mesh_ortho_numpy(V, F, tc, tn, pages, g)
        assert np.array_equal(_bits(up), _bits(T.mesh_dsm_numpy(V, F, g)))
        _, _, down = mesh_ortho_numpy(V, F, tc, tn, pages, g, z_down=True)
        mirrored = T.mesh_dsm_numpy(V * np.float32([1, 1, -1]), F, g)
        mirrored = np.where(np.isnan(mirrored), mirrored, -mirrored)   # the empty cells keep the one NaN
        assert np.array_equal(_bits(down), _bits(mirrored))
        assert np.isfinite(up).sum() > 20 and np.array_equal(np.isfinite(up), np.isfinite(down))
    # Z bounds drop samples in both modes
    gb = dsm.DsmGrid([0.0, 4.0, 0.0, 4.0, 1.0, 3.0], [1.0, 1.0])
    Vq, Fq = T.quad(0, 4, 0, 4, lambda x, y: x)
    for zd in (False, True):
        _, rgba, hb = mesh_ortho_numpy(Vq, Fq, planar_texcoords(Vq, Fq, (0, 4, 0, 4)), [0, 0], [np.full((4, 4, 3), 7, np.uint8)], gb, zd)
        assert np.array_equal(np.isfinite(hb)[0], [False, True, True, False]) and np.array_equal(rgba[0, :, 3], [0, 255, 255, 0])


def test_face_order_winding_and_corner_rotation_do_not_change_the_bits():
    g = T.grid_small()
    rng = np.random.default_rng(9)
    for zd in (False, True):
        V, F, tc, tn, pages = _field(2)
        ref = mesh_ortho_numpy(V, F, tc, tn, pages, g, zd)
        assert (ref[1][:, :, 3] == 255).sum() > 100
        p = rng.permutation(len(F))
        variants = [(F[p], tc[p], tn[p]), reverse(F, tc) + (tn,), rotate(F, tc, 1) + (tn,), rotate(F, tc, 2) + (tn,)]
        for Fv, tcv, tnv in variants:
            got = mesh_ortho_numpy(V, Fv, tcv, tnv, pages, g, zd)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(_bits(got[2]), _bits(ref[2]))
        # the rotation without the texcoords is another texture: the check above is not vacuous
        other = mesh_ortho_numpy(V, F[:, [1, 2, 0]], tc, tn, pages, g, zd)
        assert not np.array_equal(other[1], ref[1]) and np.array_equal(_bits(other[2]), _bits(ref[2]))


def _flat_pages():
    return [np.full((4, 4, 3), (10, 200, 30), np.uint8), np.full((6, 4, 3), (250, 3, 4), np.uint8)]


def _quad_tc(n=2):
    return np.tile(np.float32([0.2, 0.2, 0.8, 0.2, 0.5, 0.8]), (n, 1))


def test_two_coincident_faces_give_the_larger_colour_word():
    g = dsm.DsmGrid([0.0, 4.0, 0.0, 4.0], [1.0, 1.0])
    V, F = T.quad(0, 4, 0, 4, lambda x, y: 5.0)
    F2 = np.concatenate([F, F])
    tn = np.int32([0, 0, 1, 1])
    words = [0xff000000 | 10 | 200 << 8 | 30 << 16, 0xff000000 | 250 | 3 << 8 | 4 << 16]
    for order in ([0, 1, 2, 3], [2, 3, 0, 1], [3, 0, 2, 1]):
        for zd in (False, True):
            key, rgba, h = mesh_ortho_numpy(V, F2[order], _quad_tc(4), tn[order], _flat_pages(), g, zd)
            assert ((key & np.uint64(0xffffffff)) == max(words)).all() and (h == 5.0).all()
    assert max(words) == words[0]   # the blue byte decides: page 0's colour
    # a textured face beats an untextured coincident one
    tc = _quad_tc(4)
    tc[:2] = np.float32([0.1, 0.9] * 3)
    _, rgba, _ = mesh_ortho_numpy(V, F2, tc, np.int32([0, 0, 1, 1]), _flat_pages(), g)
    assert (rgba == np.uint8([250, 3, 4, 255])).all()


def test_an_untextured_roof_hides_the_ground_and_z_down_shows_it():
    g = dsm.DsmGrid([0.0, 8.0, 0.0, 6.0], [1.0, 1.0])
    ground = T.quad(-1, 9, -1, 7, lambda x, y: 0.0)
    roof = T.quad(2.3, 5.7, 1.6, 4.2, lambda x, y: 10.0)
    V, F = T.merge(ground, roof)
    cx, cy = np.arange(8) + 0.5, 6.0 - (np.arange(6) + 0.5)
    under = ((cx[None, :] > 2.3) & (cx[None, :] < 5.7)) & ((cy[:, None] > 1.6) & (cy[:, None] < 4.2))
    for how in ("same", "page", "nan"):
        tc = _quad_tc(4)
        tn = np.int32([0, 0, 0, 0])
        if how == "same":
            tc[2:] = np.float32([0.25, 0.75] * 3)
        elif how == "page":
            tn[2:] = [2, -1]
        else:
            tc[2, 3], tc[3, 0] = np.nan, np.inf
        _, rgba, h = mesh_ortho_numpy(V, F, tc, tn, _flat_pages(), g)
        assert (rgba[under] == 0).all() and (h[under] == 10.0).all()
        assert (rgba[~under] == np.uint8([10, 200, 30, 255])).all() and (h[~under] == 0.0).all()
        _, rgba, h = mesh_ortho_numpy(V, F, tc, tn, _flat_pages(), g, z_down=True)
        assert (rgba == np.uint8([10, 200, 30, 255])).all() and (h == 0.0).all()
    # no cell: key 0, transparent, NaN
    key, rgba, h = mesh_ortho_numpy(V, F[:0], _quad_tc(0), np.int32([]), _flat_pages(), g)
    assert (key == 0).all() and (rgba == 0).all() and np.isnan(h).all()


def test_no_finite_height_has_the_empty_key():
    z = np.float32([-3.4028235e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4028235e38])   # in the IEEE total order
    k = T.keys_of(z)
    assert (k != 0).all() and (~k != 0).all()
    assert (np.diff(k.astype(np.int64)) > 0).all() and (np.diff((~k).astype(np.int64)) < 0).all()


# ----------------------------------------------------------------------------------------
# the library, the Python layer and the command lines
# ----------------------------------------------------------------------------------------
def test_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_build_flags() == b""
    assert lib.d3d_ortho_mesh_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_ortho_mesh_scratch_bytes(1000, 30, 20) >= 30 * 20 * 8 + 1000 * 16
    assert lib.d3d_ortho_mesh_scratch_bytes(0, 30, 20) >= 30 * 20 * 8
    assert lib.d3d_ortho_mesh_scratch_bytes(5_000_000, 6000, 6000) >= 6000 * 6000 * 8 + 5_000_000 * 16
    for bad in ((-1, 30, 20), (1 << 31, 30, 20), (10, 0, 20), (10, 30, -1), (10, 1 << 16, 1 << 15)):
        assert lib.d3d_ortho_mesh_scratch_bytes(*bad) == 0, bad
    # the list constant is the mesh DSM's
    hip = open(_lib.CSRC + "/ortho_mesh.hip").read()
    assert int(re.search(r"constexpr int OM_SMALL = (\d+);", hip).group(1)) == dsm.DSM_TRI_SMALL


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below fails its checks first
    h, c, s = ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 32), ctypes.c_void_p(1 << 34)
    need = lib.d3d_ortho_mesh_scratch_bytes(10, 10, 10)
    ok = dict(v=fake, nv=30, f=fake, nf=10, tc=fake, tn=fake, atlas=fake, rows=fake, np=2, P=64, xmin=0.0, ymax=10.0, ux=1.0, uy=1.0,
              zmin=-math.inf, zmax=math.inf, W=10, H=10, zd=0, scratch=s, sbytes=need, rgba=c, height=h)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.d3d_ortho_from_mesh(a["v"], a["nv"], a["f"], a["nf"], a["tc"], a["tn"], a["atlas"], a["rows"], a["np"], a["P"], a["xmin"],
                                       a["ymax"], a["ux"], a["uy"], a["zmin"], a["zmax"], a["W"], a["H"], a["zd"], a["scratch"], a["sbytes"],
                                       a["rgba"], a["height"], None)

    cases = [(dict(v=None), b"null"), (dict(f=None), b"null"), (dict(tc=None), b"null"), (dict(tn=None), b"null"),
             (dict(atlas=None), b"null"), (dict(rows=None), b"null"), (dict(height=None), b"null"), (dict(rgba=None), b"null"),
             (dict(scratch=None), b"null"),
             (dict(nv=-1), b"n_vertices"), (dict(nv=1 << 31), b"n_vertices"), (dict(nf=-1), b"n_faces"), (dict(nf=1 << 31), b"n_faces"),
             (dict(np=0), b"n_pages"), (dict(np=-2), b"n_pages"), (dict(P=0), b"page_width"),
             (dict(W=0), b"raster"), (dict(H=0), b"raster"), (dict(W=1 << 16, H=1 << 15), b"raster"), (dict(W=-3), b"raster"),
             (dict(ux=0.0), b"unit"), (dict(uy=math.nan), b"unit"), (dict(xmin=math.inf), b"border"),
             (dict(zmin=5.0, zmax=4.0), b"z bounds"), (dict(zmin=math.nan), b"z bounds"), (dict(zd=2), b"z_down"),
             (dict(sbytes=need - 1), b"scratch"), (dict(sbytes=16), b"scratch"),
             (dict(height=ctypes.c_void_p((1 << 34) + 512)), b"alias"), (dict(rgba=ctypes.c_void_p((1 << 34) - 8)), b"alias"),
             (dict(rgba=ctypes.c_void_p((1 << 30) + 4)), b"alias")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.d3d_last_error(), (kw, lib.d3d_last_error())


def _cpu_inputs():
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    tc, tn = torch.zeros(2, 6), torch.zeros(2, dtype=torch.int32)
    atlas, rows = torch.zeros(10, 8, dtype=torch.int32), torch.tensor([0, 6, 10])
    return dict(vertices=v, faces=f, texcoord=tc, texnumber=tn, atlas=atlas, page_row=rows)


def test_operator_refuses_cpu_tensors_bad_shapes_and_a_bad_page_row():
    g = dsm.DsmGrid([0, 10, 0, 10], [1, 1])
    ok = _cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ortho_mesh.mesh_to_ortho(grid=g, **ok)
    for bad in ([[0, 1, 4], [0, 1, 2]], [[-1, 0, 1], [0, 1, 2]]):
        with pytest.raises(ValueError, match="outside"):
            ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, faces=torch.tensor(bad, dtype=torch.int32)))
    for kw, msg in ((dict(faces=ok["faces"].long()), "int32"), (dict(vertices=torch.zeros(4, 2)), r"\[n,3\]"),
                    (dict(texcoord=torch.zeros(2, 5)), "texcoord"), (dict(texcoord=torch.zeros(3, 6)), "texcoord"),
                    (dict(texcoord=torch.zeros(2, 6, dtype=torch.float64)), "texcoord"), (dict(texnumber=torch.zeros(2)), "texnumber"),
                    (dict(texnumber=torch.zeros(3, dtype=torch.int32)), "texnumber"), (dict(atlas=torch.zeros(10, 8)), "atlas"),
                    (dict(atlas=torch.zeros(80, dtype=torch.int32)), "atlas"), (dict(page_row=torch.tensor([0, 6, 10], dtype=torch.int32)), "page_row"),
                    (dict(page_row=torch.tensor([10])), "page_row"), (dict(page_row=torch.tensor([0, 6, 6, 10])), "rise"),
                    (dict(page_row=torch.tensor([0, 7, 5, 10])), "rise"), (dict(page_row=torch.tensor([1, 6, 10])), "rise"),
                    (dict(page_row=torch.tensor([0, 6, 11])), "rise")):
        with pytest.raises(ValueError, match=msg):
            ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, **kw))
    with pytest.raises(TypeError, match="DsmGrid"):
        ortho_mesh.mesh_to_ortho(grid=[0, 10, 0, 10], **ok)
    with pytest.raises(TypeError, match="Tensor"):
        ortho_mesh.mesh_to_ortho(grid=g, **dict(ok, texcoord=np.zeros((2, 6), np.float32)))


def test_atlas_from_pages_and_summary():
    pages = [np.arange(3 * 4 * 3, dtype=np.uint8).reshape(3, 4, 3), np.full((2, 4, 3), 9, np.uint8)]
    atlas, rows = ortho_mesh.atlas_from_pages(pages, 4, "cpu")
    assert atlas.dtype == torch.int32 and tuple(atlas.shape) == (5, 4) and rows.tolist() == [0, 3, 5] and rows.dtype == torch.int64
    b = atlas.numpy().view(np.uint8).reshape(5, 4, 4)
    assert np.array_equal(b[:3, :, :3], pages[0]) and (b[:, :, 3] == 255).all() and (b[3:, :, :3] == 9).all()
    for bad in ([], [np.zeros((3, 5, 3), np.uint8)], [np.zeros((3, 4, 4), np.uint8)], [np.zeros((3, 4, 3), np.float32)]):
        with pytest.raises(ValueError):
            ortho_mesh.atlas_from_pages(bad, 4, "cpu")
    rgba = torch.zeros(2, 3, 4, dtype=torch.uint8)
    height = torch.full((2, 3), float("nan"))
    height[0, :] = 1.0
    rgba[0, 0] = torch.tensor([1, 2, 3, 255], dtype=torch.uint8)
    assert ortho_mesh.summary(rgba, height) == {"cells": 6, "coloured": 1, "untextured": 2, "empty": 3}


def test_settings_and_the_module_command_line(capsys, tmp_path):
    import argparse

    ap = argparse.ArgumentParser()
    ortho_mesh.add_arguments(ap, prefix="o_")
    a = ap.parse_args(["--o_border", "0,10,0,5", "--o_size", "20,10", "--o_z_down"])
    s = ortho_mesh.settings_from_args(a, "x.tif", prefix="o_")
    assert s == {"path": "x.tif", "border": [0.0, 10.0, 0.0, 5.0], "unit": [0.1, 0.1], "size": [20, 10], "z_down": True}
    grid, zd = ortho_mesh.check_settings(s)
    assert grid.shape == (10, 20) and zd is True
    a = ap.parse_args(["--o_border", "0,10,0,5,-1,1", "--o_unit", "0.5"])
    grid, zd = ortho_mesh.check_settings(ortho_mesh.settings_from_args(a, "x.tif", prefix="o_"))
    assert grid.shape == (10, 20) and (grid.z_min, grid.z_max) == (-1.0, 1.0) and zd is False
    for bad, msg in (({"path": "x.png", "border": [0, 1, 0, 1]}, ".tif"), ({"path": "x.tif"}, "border"), ({"path": None, "border": [0, 1, 0, 1]}, ".tif"),
                     ({"path": "x.tif", "border": [0, 1, 0]}, "border"), ({"path": "x.tif", "border": [0, 1, 0, 1], "unit": [0, 1]}, "unit"),
                     ({"path": "x.tif", "border": [0, 1, 0, 1], "size": [0, 4]}, "raster"),
                     ({"path": "x.tif", "border": [0, 1, 0, 1], "z_down": "yes"}, "z_down"),
                     ({"path": "x.tif", "border": [0, 1, 0, 1], "size": [40000, 30000]}, "4 GiB")):
        with pytest.raises(ValueError, match=msg):
            ortho_mesh.check_settings(bad)
    with pytest.raises(ValueError, match="dict"):
        ortho_mesh.check_settings("x.tif")
    base = ["--textured", "t.ply", "--out", str(tmp_path / "o.tif")]
    for argv in (base, base[:2] + ["--border", "0,1,0,1"], base + ["--border", "0,1,0"], base + ["--border", "0,1,0,1", "--unit", "0,1"],
                 ["--textured", "t.ply", "--out", "o.png", "--border", "0,1,0,1"]):
        with pytest.raises(SystemExit):
            ortho_mesh.main(argv)
    err = capsys.readouterr().err
    assert "--border is required" in err and "--out" in err and ".tif" in err
    assert not (tmp_path / "o.tif").exists()


def test_predict_flags_and_their_defaults(capsys):
    base = ["--output_folder", "o", "--fuse", "--mesh", "m.ply", "--mesh_border=0,8,0,4,-1,1", "--mesh_voxel=0.1", "--texture", "t.ply"]
    a = predict.parse_args(base)
    assert a.texture_ortho is None and "ortho" not in predict._texture_settings(a)
    # the border: the mesh's footprint; the unit: 0.1
    s = predict._texture_settings(predict.parse_args(base + ["--texture_ortho", "o.tif"]))["ortho"]
    assert s == {"path": "o.tif", "border": [0.0, 8.0, 0.0, 4.0], "unit": [0.1, 0.1], "size": None, "z_down": False}
    # --dsm_border given: it is the default border; --dsm_unit only when --dsm is given
    s = predict._texture_settings(predict.parse_args(base + ["--texture_ortho", "o.tif", "--dsm_border=1,5,1,3", "--dsm_unit=0.5"]))["ortho"]
    assert s["border"] == [1.0, 5.0, 1.0, 3.0] and s["unit"] == [0.1, 0.1]
    s = predict._texture_settings(predict.parse_args(base + ["--texture_ortho", "o.tif", "--dsm", "d.tif", "--dsm_border=1,5,1,3,0,9",
                                                             "--dsm_unit=0.5,0.25"]))["ortho"]
    assert s["border"] == [1.0, 5.0, 1.0, 3.0, 0.0, 9.0] and s["unit"] == [0.5, 0.25]
    s = predict._texture_settings(predict.parse_args(base + ["--texture_ortho", "o.tif", "--dsm", "d.tif", "--dsm_border=1,5,1,3",
                                                             "--texture_ortho_border=0,2,0,2", "--texture_ortho_unit=0.2",
                                                             "--texture_ortho_size=7,9", "--texture_ortho_z_down"]))["ortho"]
    assert s == {"path": "o.tif", "border": [0.0, 2.0, 0.0, 2.0], "unit": [0.2, 0.2], "size": [7, 9], "z_down": True}
    for argv in (base[:-2] + ["--texture_ortho", "o.tif"], base + ["--texture_ortho", "o.png"],
                 base + ["--texture_ortho", "o.tif", "--texture_ortho_unit=0,1"], base + ["--texture_ortho", "o.tif", "--texture_ortho_size=0,5"],
                 base + ["--texture_ortho", "o.tif", "--texture_ortho_border=0,1,0"]):
        with pytest.raises(SystemExit):
            predict.parse_args(argv)
    err = capsys.readouterr().err
    assert "--texture_ortho needs --texture" in err and ".tif" in err
    # the texture module's own command line has no such flag: the key is absent
    import argparse

    ap = argparse.ArgumentParser()
    texture.add_arguments(ap)
    assert "ortho" not in texture.settings_from_args(ap.parse_args([]), "o.ply")
    with pytest.raises(SystemExit):
        ap.parse_args(["--ortho", "o.tif"])


def test_pipeline_validates_the_ortho_settings_up_front():
    m = {"path": "m.ply", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1}
    t = {"path": "t.ply"}
    good = {"path": "o.tif", "border": [0, 1, 0, 1], "unit": [0.1, 0.1]}
    # every error below is raised before the model or the dataset is touched
    for bad, msg in ((dict(good, path="o.png"), ".tif"), (dict(good, border=None), "border"), (dict(good, unit=[0.0, 0.1]), "unit"),
                     (dict(good, size=[0, 3]), "raster"), (dict(good, z_down=3), "z_down"), ("o.tif", "dict")):
        with pytest.raises(ValueError, match=msg):
            pipeline.predict_and_fuse(None, None, "unused", mesh=m, texture=dict(t, ortho=bad))
    with pytest.raises(ValueError, match="texture needs mesh"):
        pipeline.predict_and_fuse(None, None, "unused", texture=dict(t, ortho=good))


def test_the_kernels_use_integer_max_and_add_only_and_the_coverage_exists_once():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/ortho_mesh.hip").read())
    assert set(re.findall(r"\batomic\w*", hip)) == {"atomicMax", "atomicAdd"}
    assert not re.search(r"unsafeAtomic|atomicAdd\s*\(\s*\(?\s*(float|double)|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
    # every atomicMax is on the 64-bit keys, every atomicAdd on the list's int counter
    assert re.findall(r"atomicMax\(\s*(\w+)", hip) == ["cell"] and re.findall(r"atomicAdd\(\s*(\w+)", hip) == ["n_big"]
    assert "unsigned long long* cell" in hip and "int* __restrict__ n_big" in hip
    # the coverage primitives are defined in the shared header and nowhere else
    shared = strip(open(_lib.CSRC + "/dsm_tri.h").read())
    dsm_hip = strip(open(_lib.CSRC + "/dsm.hip").read())
    for name in ("struct DsmTri", "struct DsmGrid", "bool dsm_vtx_less(", "void dsm_vtx_swap(", "void dsm_edge(", "double dsm_edge_eval(",
                 "bool dsm_tri_setup(", "bool dsm_tri_range(", "bool dsm_tri_sample("):
        assert name in shared and name not in hip and name not in dsm_hip, name
    assert '#include "dsm_tri.h"' in hip and '#include "dsm_tri.h"' in dsm_hip
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bortho_mesh\.hip\b", make, re.M) and re.search(r"^HDRS :=.*\bdsm_tri\.h\b", make, re.M)
