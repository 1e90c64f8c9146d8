"""CPU checks of the DSM from a mesh (deep3d_aerial_amd/dsm.py mesh_to_dsm, csrc/dsm.hip; the reference's CREATEDSM step with
dsm_source "mesh", run.py:226-232, whose mesh2dsm module it never shipped).  `mesh_dsm_numpy` restates the semantics of dsm.py's
docstring in numpy; it is checked here on analytic meshes, and tests/test_dsm_mesh_gpu.py compares the kernels against it bit for
bit.  Also: the C ABI and its argument checks, the constant the Python layer mirrors, and the CLI / predict / pipeline errors."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from deep3d_aerial_amd import _lib, dsm, pipeline, predict

NEW_SYMBOLS = ("d3d_dsm_mesh_scratch_bytes", "d3d_dsm_from_mesh")


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def keys_of(z):
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _less(kp, kq):
    """Lexicographic (x, y, z) order of vertices given as total-order keys [..., 3]."""
    return (kp[:, 0] < kq[:, 0]) | ((kp[:, 0] == kq[:, 0]) & ((kp[:, 1] < kq[:, 1]) | ((kp[:, 1] == kq[:, 1]) & (kp[:, 2] < kq[:, 2]))))


def _edge(p, q):
    """(origin x, origin y, dx, dy, s) of directed edges p -> q ([m,3] fp32 each), in fp64."""
    fwd = (p[:, 0] < q[:, 0]) | ((p[:, 0] == q[:, 0]) & (p[:, 1] <= q[:, 1]))
    u = np.where(fwd[:, None], p, q).astype(np.float64)
    v = np.where(fwd[:, None], q, p).astype(np.float64)
    return u[:, 0], u[:, 1], v[:, 0] - u[:, 0], v[:, 1] - u[:, 1], np.where(fwd, 1.0, -1.0)


def triangles(vertices, faces):
    """The usable triangles of a mesh as fp64 arrays: edges (ox, oy, ex, ey, t = s sigma) [3][m] (edge k opposite vertex k), z [m,3]
    and the XY box (x_lo, x_hi, y_lo, y_hi) [m]."""
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    F = F[((F >= 0) & (F < len(V))).all(1)]
    P = V[F].copy()                                       # [m, 3 vertices, 3 coords]
    P = P[np.isfinite(P).all((1, 2))]
    for i, j in ((0, 1), (1, 2), (0, 1)):                 # lexicographic (x, y, z) order of the vertices, total order per component
        K = keys_of(P)
        sw = _less(K[:, j], K[:, i])
        a, b = P[:, i].copy(), P[:, j].copy()
        P[:, i] = np.where(sw[:, None], b, a)
        P[:, j] = np.where(sw[:, None], a, b)
    a, b, c = P[:, 0], P[:, 1], P[:, 2]
    E = [_edge(b, c), _edge(c, a), _edge(a, b)]
    ox, oy, ex, ey, s = E[2]
    with np.errstate(invalid="ignore", over="ignore"):
        D = s * (ex * (c[:, 1].astype(np.float64) - oy) - ey * (c[:, 0].astype(np.float64) - ox))
    keep = (D != 0) & np.isfinite(D)
    sigma = np.where(D > 0, 1.0, -1.0)
    edges = [(e[0][keep], e[1][keep], e[2][keep], e[3][keep], (e[4] * sigma)[keep]) for e in E]
    P = P[keep]
    box = (P[:, :, 0].min(1).astype(np.float64), P[:, :, 0].max(1).astype(np.float64), P[:, :, 1].min(1).astype(np.float64),
           P[:, :, 1].max(1).astype(np.float64))
    return edges, P[:, :, 2].astype(np.float64), box


def cell_ranges(box, grid):
    """Columns j0..j1 and rows i0..i1 whose centres a triangle is tested at (int64 [m] each), and whether the range is non-empty."""
    x_lo, x_hi, y_lo, y_hi = box
    with np.errstate(invalid="ignore", over="ignore"):
        j0 = np.maximum(np.floor((x_lo - grid.x_min) / grid.unit[0]) - 1.0, 0.0)
        j1 = np.minimum(np.floor((x_hi - grid.x_min) / grid.unit[0]) + 1.0, grid.width - 1.0)
        i0 = np.maximum(np.floor((grid.y_max - y_hi) / grid.unit[1]) - 1.0, 0.0)
        i1 = np.minimum(np.floor((grid.y_max - y_lo) / grid.unit[1]) + 1.0, grid.height - 1.0)
    ok = (j0 <= j1) & (i0 <= i1)
    as_int = lambda a: np.where(ok, a, 0).astype(np.int64)
    return as_int(j0), as_int(j1), as_int(i0), as_int(i1), ok


def mesh_dsm_numpy(vertices, faces, grid, chunk=1 << 22):
    """height [H,W] float32 (NaN where no triangle covers the centre) as dsm.py's docstring states it."""
    edges, z, box = triangles(vertices, faces)
    j0, j1, i0, i1, ok = cell_ranges(box, grid)
    nj, ni = np.where(ok, j1 - j0 + 1, 0), np.where(ok, i1 - i0 + 1, 0)
    n = nj * ni
    keymax = np.zeros(grid.width * grid.height, np.uint32)
    start = 0
    while start < len(n):                                 # triangles in groups of at most `chunk` (triangle, cell) pairs
        end, tot = start, 0
        while end < len(n) and (end == start or tot + n[end] <= chunk):
            tot += n[end]
            end += 1
        sl = slice(start, end)
        tri = np.repeat(np.arange(start, end), n[sl])
        local = np.arange(tot) - np.repeat(np.cumsum(n[sl]) - n[sl], n[sl])
        i = i0[tri] + local // nj[tri]
        j = j0[tri] + local % nj[tri]
        px = grid.x_min + (j.astype(np.float64) + 0.5) * grid.unit[0]
        py = grid.y_max - (i.astype(np.float64) + 0.5) * grid.unit[1]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            w = [e[4][tri] * (e[2][tri] * (py - e[1][tri]) - e[3][tri] * (px - e[0][tri])) for e in edges]
            W = (w[0] + w[1]) + w[2]
            cov = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (W > 0)
            zz = (((w[0] * z[tri, 0] + w[1] * z[tri, 1]) + w[2] * z[tri, 2]) / np.where(cov, W, 1.0)).astype(np.float32)
            cov &= (zz.astype(np.float64) >= grid.z_min) & (zz.astype(np.float64) <= grid.z_max)
        np.maximum.at(keymax, (i * grid.width + j)[cov], keys_of(zz[cov]))
        start = end
    h = np.where(keymax == 0, np.float32(np.nan), unkey(keymax)).astype(np.float32)
    return h.reshape(grid.shape)


# ----------------------------------------------------------------------------------------
# analytic meshes (shared with tests/test_dsm_mesh_gpu.py)
# ----------------------------------------------------------------------------------------
def quad(x0, x1, y0, y1, f):
    """Two triangles over the rectangle, heights f(x, y): (vertices [4,3], faces [2,3])."""
    xy = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return np.array([(x, y, f(x, y)) for x, y in xy], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def merge(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int32) + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def box_building(x0=2.3, x1=5.7, y0=1.6, y1=4.2, roof=10.0, ground=0.0, extent=(-1.0, 9.0, -1.0, 7.0)):
    """Ground quad, the four vertical walls and the roof of a box: (vertices, faces)."""
    g = quad(extent[0], extent[1], extent[2], extent[3], lambda x, y: ground)
    r = quad(x0, x1, y0, y1, lambda x, y: roof)
    walls = []
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    for k in range(4):
        (ax, ay), (bx, by) = c[k], c[(k + 1) % 4]
        walls.append((np.array([(ax, ay, ground), (bx, by, ground), (bx, by, roof), (ax, ay, roof)], np.float32),
                      np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
    return merge(g, r, *walls)


def height_field(n=24, seed=0, spacing=1.0, origin=0.5, jitter=0.3):
    """A triangulated height field on an n x n lattice (x = origin + k spacing), each quad cut along a random diagonal; interior
    vertices are jittered (half of them stay on the lattice), boundary ones are not, so the footprint is the lattice's square."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    X, Y = np.meshgrid(origin + k * spacing, origin + k * spacing)
    inner = (np.arange(n)[None, :] > 0) & (np.arange(n)[None, :] < n - 1) & (np.arange(n)[:, None] > 0) & (np.arange(n)[:, None] < n - 1)
    move = inner & (rng.uniform(size=(n, n)) < 0.5)
    X = np.where(move, X + rng.uniform(-jitter, jitter, (n, n)) * spacing, X)
    Y = np.where(move, Y + rng.uniform(-jitter, jitter, (n, n)) * spacing, Y)
    Z = np.sin(X * 0.4) * 3 + np.cos(Y * 0.3) * 2 + rng.uniform(0, 0.5, (n, n))
    V = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    F = []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, d, e = r * n + c, r * n + c + 1, (r + 1) * n + c + 1, (r + 1) * n + c
            F += [[a, b, d], [a, d, e]] if rng.uniform() < 0.5 else [[a, b, e], [b, d, e]]
    return V, np.array(F, np.int32)


def soup(n, seed, extent=(-5.0, 25.0, -5.0, 20.0), size=3.0, big=False):
    """Random triangles, partly outside the raster, with degenerate, vertical and non-finite ones mixed in."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(extent[0], extent[1], n), rng.uniform(extent[2], extent[3], n), rng.uniform(-5, 15, n)], -1)
    s = size * (8.0 if big else 1.0)
    V = (c[:, None, :] + rng.uniform(-s, s, (n, 3, 3)) * [1, 1, 0.5]).astype(np.float32)
    k = rng.integers(0, 20, n)
    V[k == 0, 1] = V[k == 0, 0]                                             # two equal vertices
    V[k == 1, 2, :2] = V[k == 1, 0, :2]                                     # vertical: two vertices share x, y
    V[k == 2, 2, :2] = (V[k == 2, 0, :2] + V[k == 2, 1, :2]) * np.float32(0.5)   # collinear in xy (up to rounding)
    V[k == 3, 1, 2] = np.nan
    V[k == 4, 0, 0] = np.inf
    return V.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def grid_small():
    return dsm.DsmGrid([0.0, 20.0, 0.0, 15.0], [0.5, 0.5])


# ----------------------------------------------------------------------------------------
def test_a_tilted_plane_as_two_triangles_is_the_plane_at_every_centre():
    g = dsm.DsmGrid([0.0, 12.0, 0.0, 9.0], [0.25, 0.5])
    f = lambda x, y: 0.3 * x - 0.7 * y + 20.0
    V, F = quad(-1.0, 13.0, -2.0, 10.0, f)
    h = mesh_dsm_numpy(V, F, g)
    cx = g.x_min + (np.arange(g.width) + 0.5) * g.unit[0]
    cy = g.y_max - (np.arange(g.height) + 0.5) * g.unit[1]
    want = f(cx[None, :], cy[:, None]).astype(np.float32)
    assert not np.isnan(h).any()
    assert (np.abs(h - want) <= 2 * np.spacing(np.abs(want))).all(), np.abs(h - want).max()
    # the diagonal passes through centres: both triangles sample there, and the larger sample in total order wins
    V2, F2 = quad(0.0, 12.0, 0.0, 9.0, f)
    assert not np.isnan(mesh_dsm_numpy(V2, F2, g)).any()   # the quad's edges lie on the raster's border: centres inside


def test_a_box_building_gives_the_roof_inside_its_footprint_and_the_ground_outside():
    g = dsm.DsmGrid([0.0, 8.0, 0.0, 6.0], [1.0, 1.0])
    V, F = box_building()
    h = mesh_dsm_numpy(V, F, g)
    cx = np.arange(8) + 0.5
    cy = 6.0 - (np.arange(6) + 0.5)
    inside = ((cx[None, :] > 2.3) & (cx[None, :] < 5.7)) & ((cy[:, None] > 1.6) & (cy[:, None] < 4.2))
    assert inside.sum() == 8
    assert (h[inside] == 10.0).all() and (h[~inside] == 0.0).all()
    # the walls alone are vertical: nothing
    walls = (V, F[4:])
    assert np.isnan(mesh_dsm_numpy(*walls, g)).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_jittered_height_field_has_no_hole_inside_its_footprint(seed):
    # lattice vertices on cell centres: centres fall exactly on shared edges (lattice rows and columns) and on vertices
    g = dsm.DsmGrid([0.0, 24.0, 0.0, 24.0], [1.0, 1.0])
    V, F = height_field(24, seed)
    h = mesh_dsm_numpy(V, F, g)
    assert not np.isnan(h).any()          # the footprint [0.5, 23.5]^2 holds every centre, its border included
    # a finer raster: several centres per triangle, and centres on the diagonals
    g2 = dsm.DsmGrid([0.5, 23.5, 0.5, 23.5], [0.25, 0.25])
    h2 = mesh_dsm_numpy(V, F, g2)
    assert not np.isnan(h2).any()
    assert np.nanmin(h2) >= V[:, 2].min() and np.nanmax(h2) <= V[:, 2].max()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_winding_vertex_order_and_triangle_order_do_not_change_the_bits():
    g = grid_small()
    rng = np.random.default_rng(5)
    for V, F in (height_field(16, 3, spacing=1.1, origin=0.3), soup(400, 4), box_building()):
        ref = mesh_dsm_numpy(V, F, g)
        assert np.isfinite(ref).sum() > 20
        assert np.array_equal(_bits(mesh_dsm_numpy(V, F[:, ::-1], g)), _bits(ref))
        assert np.array_equal(_bits(mesh_dsm_numpy(V, F[:, [1, 2, 0]], g)), _bits(ref))
        assert np.array_equal(_bits(mesh_dsm_numpy(V, F[rng.permutation(len(F))], g)), _bits(ref))
        # the vertex list renumbered
        p = rng.permutation(len(V))
        inv = np.argsort(p)
        assert np.array_equal(_bits(mesh_dsm_numpy(V[p], inv[F].astype(np.int32), g)), _bits(ref))


def test_vertical_degenerate_and_non_finite_triangles_and_z_bounds():
    g = dsm.DsmGrid([0.0, 4.0, 0.0, 4.0], [1.0, 1.0])
    V = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1],      # covers the lower-left half at z = 1
                  [1, 1, 0], [3, 3, 0], [1, 1, 9],      # vertical
                  [0, 0, 7], [4, 4, 7], [2, 2, 7],      # collinear in xy
                  [0, 0, 8], [0, 0, 8], [4, 4, 8],      # two equal vertices
                  [0, 0, np.nan], [4, 0, 9], [0, 4, 9],  # non-finite
                  [0, 0, np.inf], [4, 0, 9], [0, 4, 9]], np.float32)
    F = np.arange(18, dtype=np.int32).reshape(6, 3)
    h = mesh_dsm_numpy(V, F, g)
    assert np.array_equal(np.isfinite(h), np.tril(np.ones((4, 4), bool)))   # centres with x + y <= 4 (row 0 north)
    assert (h[np.isfinite(h)] == 1.0).all()
    assert np.isnan(mesh_dsm_numpy(V, F[1:], g)).all()
    # out-of-range indices contribute nothing here (mesh_to_dsm refuses them before a launch)
    assert np.array_equal(_bits(mesh_dsm_numpy(V, np.concatenate([F, [[0, 1, 99], [-1, 0, 1]]]).astype(np.int32), g)), _bits(h))
    # Z bounds drop samples, not triangles: a tilted plane from z = 0 to 4 keeps the centres inside [1, 3]
    f = lambda x, y: x
    Vq, Fq = quad(0, 4, 0, 4, f)
    hb = mesh_dsm_numpy(Vq, Fq, dsm.DsmGrid([0.0, 4.0, 0.0, 4.0, 1.0, 3.0], [1.0, 1.0]))
    assert np.array_equal(np.isfinite(hb)[0], [False, True, True, False]) and np.array_equal(hb[:, 1], np.full(4, 1.5, np.float32))
    # overlapping surfaces: the larger sample wins, -0.0 < +0.0
    Vz = np.array([[0, 0, -0.0], [8, 0, -0.0], [0, 8, -0.0], [0, 0, 0.0], [8, 0, 0.0], [0, 8, 0.0]], np.float32)
    hz = mesh_dsm_numpy(Vz, np.array([[0, 1, 2]], np.int32), g)
    assert np.signbit(hz[np.isfinite(hz)]).all()
    hz = mesh_dsm_numpy(Vz, np.array([[0, 1, 2], [3, 4, 5]], np.int32), g)
    assert not np.signbit(hz[np.isfinite(hz)]).any()


def test_cell_ranges_cover_every_centre_of_the_box_with_a_margin():
    g = dsm.DsmGrid([-3.0, 7.0, -2.0, 6.0], [0.5, 0.4])
    rng = np.random.default_rng(1)
    for _ in range(200):
        x = np.sort(rng.uniform(-5, 9, 2))
        y = np.sort(rng.uniform(-4, 8, 2))
        j0, j1, i0, i1, ok = cell_ranges((x[:1], x[1:], y[:1], y[1:]), g)
        cx = g.x_min + (np.arange(g.width) + 0.5) * g.unit[0]
        cy = g.y_max - (np.arange(g.height) + 0.5) * g.unit[1]
        js = np.flatnonzero((cx >= x[0]) & (cx <= x[1]))
        iis = np.flatnonzero((cy >= y[0]) & (cy <= y[1]))
        if len(js) and len(iis):
            assert ok[0] and j0[0] <= js.min() - (js.min() > 0) and j1[0] >= js.max() + (js.max() < g.width - 1)
            assert i0[0] <= iis.min() - (iis.min() > 0) and i1[0] >= iis.max() + (iis.max() < g.height - 1)


# ----------------------------------------------------------------------------------------
# the library, the Python layer and the command lines
# ----------------------------------------------------------------------------------------
def test_header_binding_library_and_mirrored_constant():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    hip = open(_lib.CSRC + "/dsm.hip").read()
    assert int(re.search(r"constexpr int DSM_TRI_SMALL = (\d+);", hip).group(1)) == dsm.DSM_TRI_SMALL
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_dsm_mesh_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_dsm_mesh_scratch_bytes(1000, 30, 20) >= 30 * 20 * 4 + 1000 * 16
    assert lib.d3d_dsm_mesh_scratch_bytes(0, 30, 20) >= 30 * 20 * 4
    for bad in ((-1, 30, 20), (1 << 31, 30, 20), (10, 0, 20), (10, 30, -1), (10, 1 << 16, 1 << 15)):
        assert lib.d3d_dsm_mesh_scratch_bytes(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below fails its checks first
    h, s = ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 34)
    need = lib.d3d_dsm_mesh_scratch_bytes(10, 10, 10)
    ok = dict(v=fake, nv=30, f=fake, nf=10, xmin=0.0, ymax=10.0, ux=1.0, uy=1.0, zmin=-math.inf, zmax=math.inf, W=10, H=10, scratch=s,
              sbytes=need, height=h)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.d3d_dsm_from_mesh(a["v"], a["nv"], a["f"], a["nf"], a["xmin"], a["ymax"], a["ux"], a["uy"], a["zmin"], a["zmax"],
                                     a["W"], a["H"], a["scratch"], a["sbytes"], a["height"], None)

    cases = [(dict(v=None), b"null"), (dict(f=None), b"null"), (dict(height=None), b"null"), (dict(scratch=None), b"null"),
             (dict(nv=-1), b"n_vertices"), (dict(nv=1 << 31), b"n_vertices"), (dict(nf=-1), b"n_faces"), (dict(nf=1 << 31), b"n_faces"),
             (dict(W=0), b"raster"), (dict(H=0), b"raster"), (dict(W=1 << 16, H=1 << 15), b"raster"), (dict(W=-3), b"raster"),
             (dict(ux=0.0), b"unit"), (dict(uy=math.nan), b"unit"), (dict(xmin=math.inf), b"border"),
             (dict(zmin=5.0, zmax=4.0), b"z bounds"), (dict(zmin=math.nan), b"z bounds"),
             (dict(sbytes=need - 1), b"scratch"), (dict(sbytes=16), b"scratch"),
             (dict(height=ctypes.c_void_p((1 << 34) + 512)), b"alias"), (dict(height=ctypes.c_void_p((1 << 34) - 8)), b"alias"),
             (dict(scratch=ctypes.c_void_p((1 << 30) + 4)), b"alias")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.d3d_last_error(), (kw, lib.d3d_last_error())


def test_operator_refuses_cpu_tensors_bad_indices_and_bad_settings():
    g = dsm.DsmGrid([0, 10, 0, 10], [1, 1])
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsm.mesh_to_dsm(v, f, g)
    for bad in ([[0, 1, 4]], [[-1, 0, 1]], [[0, 1, 2], [3, 2, 7]]):
        with pytest.raises(ValueError, match="outside"):
            dsm.mesh_to_dsm(v, torch.tensor(bad, dtype=torch.int32), g)
    with pytest.raises(ValueError, match="int32"):
        dsm.mesh_to_dsm(v, f.long(), g)
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        dsm.mesh_to_dsm(torch.zeros(4, 2), f, g)
    with pytest.raises(ValueError, match="interpolation"):
        dsm.mesh_to_dsm(v, f, g, interpolation="Kriging")
    with pytest.raises(ValueError, match="radius"):
        dsm.mesh_to_dsm(v, f, g, interpolation="MovingAverage", radius=0)
    with pytest.raises(TypeError, match="DsmGrid"):
        dsm.mesh_to_dsm(v, f, [0, 10, 0, 10])
    for bad in ({"select": "Robust_Max"}, {"min_points": 2}):
        with pytest.raises(ValueError, match="mesh"):
            dsm.check_mesh_settings(bad)
    dsm.check_mesh_settings({"select": "Max", "min_points": 1, "trim": 0.3})


def test_dsm_command_line_takes_one_source(capsys, tmp_path):
    base = ["--out", str(tmp_path / "d.tif"), "--border", "0,10,0,10", "--unit", "1"]
    for argv in (base, base + ["--fused", "x", "--mesh", "m.ply"], base + ["--mesh", "m.ply", "--select", "Robust_Max"],
                 base + ["--mesh", "m.ply", "--min_points", "2"]):
        with pytest.raises(SystemExit):
            dsm.main(argv)
    err = capsys.readouterr().err
    assert "one of the arguments --fused --mesh is required" in err and "not allowed with argument" in err
    assert "--select Max" in err and "--min_points" in err


def test_predict_dsm_source_flag():
    base = ["--output_folder", "o", "--fuse", "--dsm", "x.tif", "--dsm_border=0,1,0,1"]
    a = predict.parse_args(base)
    assert a.dsm_source == "pc" and "source" not in predict._dsm_settings(a)
    mesh_flags = ["--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.1"]
    b = predict.parse_args(base + mesh_flags + ["--dsm_source", "mesh", "--dsm_interpolation", "MovingAverage"])
    s = predict._dsm_settings(b)
    assert s["source"] == "mesh" and s["interpolation"] == "MovingAverage" and s["select"] == "Max"
    for extra in (["--dsm_source", "mesh"], mesh_flags + ["--dsm_source", "mesh", "--dsm_select", "Robust_Max"],
                  mesh_flags + ["--dsm_source", "mesh", "--dsm_min_points", "3"], ["--dsm_source", "tin"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + extra)
    from deep3d_aerial_amd import mvs_dl

    flags = mvs_dl.dsm_flags(dict(s, path="x.tif"))
    assert "--dsm_source=mesh" in flags and not any(f.startswith("--dsm_source") for f in mvs_dl.dsm_flags(dict(s, path="x.tif", source="pc")))


def test_pipeline_validates_a_mesh_dsm_up_front():
    d = {"path": "x.tif", "border": [0, 1, 0, 1], "unit": [0.1, 0.1], "source": "mesh"}
    m = {"path": "m.ply", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1}
    # every error below is raised before the model or the dataset is touched
    for kw, msg in ((dict(dsm=d), "mesh settings"), (dict(dsm=dict(d, select="Robust_Max"), mesh=m), "Max"),
                    (dict(dsm=dict(d, min_points=2), mesh=m), "min_points"), (dict(dsm=dict(d, source="tin"), mesh=m), "source")):
        with pytest.raises(ValueError, match=msg):
            pipeline.predict_and_fuse(None, None, "unused", **kw)
