"""The point-to-plane metric of the registration without a GPU (deep3d_aerial_amd/cloud_register.py plane_sums / solve_plane /
register(metric="plane"), csrc/cloud_register.hip): the 87 sums restated in numpy and Python integers, the limb
recombination, solve_plane on exact motions of a curved surface and of a flat one, the header and the binding, the entry point's and
the front end's refusals, the command line.

`plane_sums_numpy` is the rule on points; `plane_sums_from_bins` the rule on the integers a, b, m it derives: per counted pair
u = a - c, r = (a - b) . m, w = u x m, g = (w, m); slots [0] N, [1] sum e, [2] sum e^2, then the 28 products -- 21 g_i g_j (i <= j,
row-major), 6 g_i r, r r -- as 128-bit two's-complement values in three slots each: the low and the high 32 bits of the low word,
unsigned, and the signed high word."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import cloud_register_scene as S
import test_cloud as TC
from deep3d_aerial_amd import _lib, cloud, cloud_register as CR

NEW_SYMBOLS = ("d3d_cloud_register_plane_sums",)
M32 = 0xFFFFFFFF


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def _limbs(p):
    """The three slots of one product (a Python integer): low 32, next 32 (unsigned), the signed high word."""
    lo = p & ((1 << 64) - 1)
    return [lo & M32, lo >> 32, p >> 64]


def plane_sums_from_bins(a, b, m, c, e):
    """The 87 sums as a list of Python integers from a, b, m [N,3] int64 of the counted pairs, c (3 integers) and e [N].  Up to
    5000 pairs every product is a Python integer; beyond, the 128-bit products are built from 32-bit halves in int64, where no slot
    can overflow -- the two routes are checked against each other."""
    a, b, m = (np.asarray(v, np.int64).reshape(-1, 3) for v in (a, b, m))
    e = np.asarray(e, np.int64)
    u = a - np.asarray(c, np.int64)
    r = ((a - b) * m).sum(1)
    w = np.stack([u[:, 1] * m[:, 2] - u[:, 2] * m[:, 1], u[:, 2] * m[:, 0] - u[:, 0] * m[:, 2], u[:, 0] * m[:, 1] - u[:, 1] * m[:, 0]], 1)
    g = np.concatenate([w, m, r[:, None]], 1)                  # |g| < 2^43: the int64 arithmetic above is exact
    assert g.size == 0 or np.abs(g).max() < 1 << 43
    pairs = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(7)]
    out = [len(a), int(e.sum()), int((e * e).sum())]
    if len(a) <= 5000:
        G = g.tolist()
        for i, j in pairs:
            limbs = [_limbs(row[i] * row[j]) for row in G]
            out += [sum(t[k] for t in limbs) for k in range(3)]
        return out
    for i, j in pairs:
        x, y = g[:, i], g[:, j]
        x0, x1, y0, y1 = x & M32, x >> 32, y & M32, y >> 32          # x = x1 2^32 + x0, x0 unsigned, x1 signed and small
        low = x0 * y0                                                # < 2^64: wraps as an int64, read through uint64
        mid = x0 * y1 + x1 * y0                                      # |mid| < 2^45
        lo64 = (x * y).view(np.uint64)                               # the product mod 2^64
        carry = ((low.view(np.uint64) >> np.uint64(32)).astype(np.int64) + (mid & M32)) >> 32
        hi = x1 * y1 + (mid >> 32) + carry
        out += [int((lo64 & np.uint64(M32)).astype(np.int64).sum()), int((lo64 >> np.uint64(32)).astype(np.int64).sum()), int(hi.sum())]
    return out


def plane_sums_numpy(moved, e, idx, reference, normals, grid, e_max=1024):
    """The 87 sums of the pairs (moved[i], reference[idx[i]]) that count: 0 <= idx < len(reference), e <= e_max, and a normal
    that is finite with every |component| <= 1 and m = rint(normal * 1024) != 0."""
    moved, reference = np.asarray(moved, np.float32).reshape(-1, 3), np.asarray(reference, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    e, idx = np.asarray(e, np.int64), np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < len(reference)) & (e <= e_max)
    if not len(reference):
        return [0] * 87
    with np.errstate(invalid="ignore", over="ignore"):
        nd = normals[np.where(ok, idx, 0)].astype(np.float64) * 1024.0
        ok &= (np.abs(nd) <= 1024.0).all(1)      # false for a NaN and an inf
    m = np.rint(np.where(ok[:, None], nd, 0.0)).astype(np.int64)
    ok &= (m != 0).any(1)
    a, b = S.bins_numpy(moved[ok], grid), S.bins_numpy(reference[idx[ok]], grid)
    return plane_sums_from_bins(a, b, m[ok], [512 * k for k in grid.n], e[ok])


def products_direct(a, b, m, c):
    """(H, v, rr) in Python integers, straight from the definition."""
    H, v, rr = [[0] * 6 for _ in range(6)], [0] * 6, 0
    for A, B, Mv in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(m).tolist()):
        u = [A[k] - c[k] for k in range(3)]
        r = sum((A[k] - B[k]) * Mv[k] for k in range(3))
        g = [u[1] * Mv[2] - u[2] * Mv[1], u[2] * Mv[0] - u[0] * Mv[2], u[0] * Mv[1] - u[1] * Mv[0]] + Mv
        for i in range(6):
            v[i] += g[i] * r
            for j in range(6):
                H[i][j] += g[i] * g[j]
        rr += r * r
    return H, v, rr


# ----------------------------------------------------------------------------------------
# the sums and their limbs
# ----------------------------------------------------------------------------------------
def far_corner_bins():
    """Pairs at the far corner of the largest grid, a = 2^31 - 1 on every axis, with normals of either sign: w reaches 2^41 and
    the products 2^83, of both signs."""
    top = (1 << 31) - 1
    a = np.int64([[top, top, top], [top, top - 5, top], [top, top, top - 1000], [top - 7, top, top]])
    b = np.int64([[top - 900, top, top - 30], [top, top, top - 1024], [0, 0, 0], [top, 5, top]])
    m = np.int64([[1024, 0, 0], [-724, 724, 0], [0, -1024, 1], [591, 591, -591]])
    return a, b, m, [0, 0, 0]


def test_the_limb_recombination_round_trips_products_of_both_signs_at_the_far_corner():
    a, b, m, c = far_corner_bins()
    s = plane_sums_from_bins(a, b, m, c, [0, 1, 2, 1024])
    assert len(s) == 87 and s[:3] == [4, 1027, 1 + 4 + 1024 * 1024]
    H, v, rr = CR.plane_products(s)
    assert (H, v, rr) == products_direct(a, b, m, c)
    flat = [H[i][j] for i in range(6) for j in range(i, 6)] + v + [rr]
    assert max(flat) > 1 << 83 and min(flat) < -(1 << 83)                 # the high word is in use, with either sign
    assert min(s[5::3]) < 0 < max(s[5::3]) and all(0 <= x < 4 << 32 for k in (3, 4) for x in s[k::3])
    # a single negative product: -1 is all ones in the two low slots and -1 in the high one
    one = plane_sums_from_bins([[3, 0, 0]], [[4, 0, 0]], [[1, 0, 0]], [0, 0, 0], [7])     # r = -1, g = (0, 0, 0, 1, 0, 0)
    P = lambda i: one[3 + 3 * i:6 + 3 * i]
    assert P(24) == [M32, M32, -1] and P(27) == [1, 0, 0] and CR.plane_products(one)[1][3] == -1 and CR.plane_products(one)[2] == 1
    assert CR.plane_products(torch.tensor(one)) == CR.plane_products(one)
    for bad in ([0] * 27, [0] * 88):
        with pytest.raises(ValueError, match="87"):
            CR.plane_products(bad)


def test_the_two_routes_of_the_restatement_agree():
    rng = np.random.default_rng(0)
    top = (1 << 31) - 1
    a, b = rng.integers(0, top, (5001, 3)), rng.integers(0, top, (5001, 3))
    m = rng.integers(-1024, 1025, (5001, 3))
    e = rng.integers(0, 1025, 5001)
    c = [512 * 1000, 512 * ((1 << 21) - 1), 512]
    big = plane_sums_from_bins(a, b, m, c, e)
    small = [plane_sums_from_bins(a[k:k + 2500], b[k:k + 2500], m[k:k + 2500], c, e[k:k + 2500]) for k in (0, 2500, 5000)]
    assert big == [sum(t) for t in zip(*small)]
    assert min(big[5::3]) < 0 < max(big[5::3])


def test_pairs_that_do_not_count_in_the_restatement():
    g = TC.unit_grid(8, 8, 8)
    moved = np.float32([[1.5, 1.5, 1.5]] * 8)
    ref = np.float32([[1.25, 1.5, 1.5]] * 8)
    nrm = np.float32([[0, 0, 1], [0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, 1.5, 0], [1e-4, 0, 0], [0, 0, -1], [0.6, 0, 0.8]])
    idx = np.arange(8, dtype=np.int32)
    e = np.full(8, 256, np.int32)
    counted = [plane_sums_numpy(moved[k:k + 1], e[k:k + 1], idx[:1], ref[:1], nrm[k:k + 1], g)[0] for k in range(8)]
    assert counted == [1, 0, 0, 0, 0, 0, 1, 1]                    # zero, NaN, inf, longer than a unit normal, rounds to zero
    assert plane_sums_numpy(moved, e, idx, ref, nrm, g)[0] == 3
    assert plane_sums_numpy(moved, e, np.int32([-1, 8, 0, 0, 0, 0, 0, 0]), ref, nrm, g)[0] == 6
    assert plane_sums_numpy(moved, e, idx, ref, nrm, g, e_max=255)[0] == 0
    assert plane_sums_numpy(moved[:0], e[:0], idx[:0], ref, nrm, g) == [0] * 87 == plane_sums_numpy(moved, e, idx - 9, ref[:0], nrm[:0], g)


# ----------------------------------------------------------------------------------------
# solve_plane
# ----------------------------------------------------------------------------------------
EXTENT = 32.0
FINE = cloud.CloudGrid(S.BORDER, 2.0 ** -15)      # 2^20 cells on the long axes: one bin is 2^-25, below 1e-9 of the extent


def _bins(p, grid):
    """Exact world points [n,3] float64 -> bins (the rule's rint, without the fp32 rounding of a stored cloud)."""
    o = np.array(grid.border[0::2])
    return np.rint((p - o) / grid.voxel * 1024.0).astype(np.int64)


def _motion(degrees, shift):
    """A rotation by `degrees` about the axis (1, -2, 3) around the border's centre, then the shift."""
    k = np.array([1.0, -2.0, 3.0]) / math.sqrt(14.0)
    t = math.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    c = np.array([16.0, 16.0, 8.0])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, c - R @ c + np.asarray(shift, np.float64)
    return M


def _smooth(n, seed):
    """n points of the smooth part of the scene's heightfield with their exact unit normals."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(4, 28, n), rng.uniform(4, 28, n)
    z = 4.0 + 1.5 * np.sin(0.45 * x) * np.cos(0.3 * y) + 0.08 * x
    nrm = np.stack([-(1.5 * 0.45 * np.cos(0.45 * x) * np.cos(0.3 * y) + 0.08), 1.5 * 0.3 * np.sin(0.45 * x) * np.sin(0.3 * y), np.ones(n)], 1)
    return np.stack([x, y, z], 1), nrm / np.sqrt((nrm * nrm).sum(1))[:, None]


def _iterate(points, normals, M, steps, grid=FINE):
    """solve_plane on the true pairs (M p, p) with the normals of p, `steps` times: [(T, info)] after every step."""
    b, m = _bins(points, grid), np.rint(normals * 1024.0).astype(np.int64)
    c = [512 * k for k in grid.n]
    T, out = np.eye(4), []
    for _ in range(steps):
        A = T @ M
        a = _bins(points @ A[:3, :3].T + A[:3, 3], grid)
        dT, info = CR.solve_plane(plane_sums_from_bins(a, b, m, c, np.zeros(len(a), np.int64)), grid)
        assert dT is not None and not info["degenerate"]
        T = dT @ T
        out.append((T, info))
    return out


def test_an_exact_small_motion_of_a_curved_surface_is_recovered():
    """The first step is right to first order: what it leaves is second order in the motion, below rotation x displacement x 2
    (the neglected terms are the products of the rotation with the displacement it causes and with the shift).  After three steps
    the error is the quantisation's: below 1e-9 of the extent, about one bin of the fine grid."""
    points, normals = _smooth(2000, 1)
    M = _motion(0.4, (0.05, -0.04, 0.03))
    truth = np.linalg.inv(M)
    moved0 = CR.corner_motion(M, S.BORDER)
    steps = _iterate(points, normals, M, 3)
    errs = [S.corner_error(T, truth) for T, _ in steps]
    print("moved %.4g, corner error after each step %s, plane_rms %s" % (moved0, errs, [i["plane_rms"] for _, i in steps]))
    assert errs[0] < 2.0 * math.radians(0.4) * moved0 and errs[0] < moved0 / 20
    assert errs[2] < 1e-9 * EXTENT
    assert [i["rank"] for _, i in steps] == [6, 6, 6] and all(i["pairs"] == 2000 and i["rms"] == 0.0 for _, i in steps)
    assert steps[0][1]["plane_rms"] > 100 * steps[2][1]["plane_rms"]


def test_a_flat_plane_has_rank_three_and_leaves_x_y_and_yaw_alone():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(4, 28, 500), rng.uniform(4, 28, 500)
    points = np.stack([x, y, np.full(500, 5.0)], 1)
    normals = np.tile([0.0, 0.0, 1.0], (500, 1))
    M = _motion(0.4, (0.05, -0.04, 0.03))
    (T, info), = _iterate(points, normals, M, 1)
    assert info["rank"] == 3 and not info["degenerate"]
    c = np.array([16.0, 16.0, 8.0])
    assert np.abs((T[:3, :3] @ c + T[:3, 3] - c)[:2]).max() <= 1e-9 * EXTENT       # the grid's centre does not move in x or y
    assert abs(T[1, 0] - T[0, 1]) * EXTENT <= 1e-9 * EXTENT                          # no rotation about z
    assert abs((T[:3, :3] @ c + T[:3, 3] - c)[2]) > 0.01                             # z, roll and pitch are solved
    # a tilted plane: the same rank, though no unknown's column is zero; the step brings the points back onto the plane to first order
    tilt = np.array([0.3, -0.2, 1.0]) / math.sqrt(1.13)
    points = np.stack([x, y, 6.0 - (tilt[0] * (x - 16) + tilt[1] * (y - 16)) / tilt[2]], 1)
    (T, info), = _iterate(points, np.tile(tilt, (500, 1)), M, 1)
    assert info["rank"] == 3
    A = T @ M
    off = np.abs(((points @ A[:3, :3].T + A[:3, 3]) - points) @ tilt).max()
    before = np.abs(((points @ M[:3, :3].T + M[:3, 3]) - points) @ tilt).max()
    assert off < 2.0 * math.radians(0.4) * CR.corner_motion(M, S.BORDER) and off < before / 20


def test_fewer_than_six_pairs_and_empty_sums_are_degenerate():
    points, normals = _smooth(5, 3)
    grid = FINE
    b, m = _bins(points, grid), np.rint(normals * 1024.0).astype(np.int64)
    s = plane_sums_from_bins(b + 3, b, m, [512 * k for k in grid.n], [5] * 5)
    dT, info = CR.solve_plane(s, grid)
    assert dT is None and info["degenerate"] and info["pairs"] == 5 and info["rank"] == 0 and info["plane_rms"] > 0
    assert info["rms"] == 5 / 1024 * grid.voxel
    dT, info = CR.solve_plane([0] * 87, grid)
    assert dT is None and info == {"pairs": 0, "rms": 0.0, "plane_rms": 0.0, "rank": 0, "degenerate": True}
    for bad, msg in (([0] * 27, "87"), ([-1] + [0] * 86, "pairs")):
        with pytest.raises(ValueError, match=msg):
            CR.solve_plane(bad, grid)
    for ratio in (0, 1, -1e-6, math.nan, "1e-6"):
        with pytest.raises(ValueError, match="min_eig_ratio"):
            CR.solve_plane([0] * 87, grid, ratio)
    with pytest.raises(TypeError, match="CloudGrid"):
        CR.solve_plane([0] * 87, S.BORDER)


# ----------------------------------------------------------------------------------------
# the library, the operator, the front end and the command line
# ----------------------------------------------------------------------------------------
def test_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and len(_lib.SIGNATURES[s]) == 17
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    assert sorted(_lib.STRUCTS) == ["d3d_mesh_grid_t", "d3d_mesh_view_t", "d3d_ortho_view_t"]   # no new struct
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    assert CR.PLANE_SUMS == 87 and CR.METRICS == ("point", "plane")


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    ok = dict(q=P(1), e=P(2), idx=P(3), nq=10, t=P(4), tn=P(5), nt=7, nx=16, ny=8, nz=4, x=0.0, y=1.0, z=-2.0, h=0.5, emax=1024, sums=P(6), st=None)
    order = ["q", "e", "idx", "nq", "t", "tn", "nt", "nx", "ny", "nz", "x", "y", "z", "h", "emax", "sums", "st"]
    TC._expect(lib, lib.d3d_cloud_register_plane_sums, ok, order,
               [(dict([(name, None)]), b"null") for name in ("q", "e", "idx", "t", "tn", "sums")] +
               [(dict(nq=-1), b"n_query"), (dict(nq=1 << 31), b"n_query"), (dict(nt=-1), b"n_target"), (dict(nt=1 << 31), b"n_target"),
                (dict(nx=0), b"grid"), (dict(ny=1 << 21), b"grid"), (dict(nz=-3), b"grid"), (dict(x=math.nan), b"origin"), (dict(z=math.inf), b"origin"),
                (dict(h=0.0), b"cap"), (dict(h=math.nan), b"cap"), (dict(emax=-1), b"e_max"), (dict(emax=1025), b"e_max"),
                (dict(tn=P(4)), b"alias"), (dict(tn=ctypes.c_void_p((4 << 32) + 83)), b"alias"), (dict(sums=ctypes.c_void_p((5 << 32) + 80)), b"alias"),
                (dict(q=ctypes.c_void_p((6 << 32) + 695)), b"alias"), (dict(idx=ctypes.c_void_p((2 << 32) + 36)), b"alias")])
    for kw in (dict(nq=0, q=None, e=None, idx=None), dict(nt=0, t=None, tn=None)):
        a = dict(ok, **kw)
        assert lib.d3d_cloud_register_plane_sums(*[a[k] for k in order[:-2]], None, None) == -1      # sums is always needed


def test_the_operator_and_the_front_end_refuse_bad_arguments():
    g = TC.unit_grid()
    xyz, nrm = torch.zeros(5, 3), torch.zeros(5, 3)
    e = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.plane_sums(xyz, e, e, xyz, nrm, g)
    with pytest.raises(ValueError, match="reference_normals"):
        CR.plane_sums(xyz, e, e, xyz, None, g)
    for bad in (nrm.double(), torch.zeros(5, 2), torch.zeros(4, 3)):
        with pytest.raises(ValueError, match="reference_normals"):
            CR.plane_sums(xyz, e, e, xyz, bad, g)
    with pytest.raises(TypeError, match="Tensor"):
        CR.plane_sums(xyz, e, e, xyz, np.zeros((5, 3), np.float32), g)
    with pytest.raises(ValueError, match="e_max"):
        CR.plane_sums(xyz, e, e, xyz, nrm, g, 1025)
    with pytest.raises(TypeError, match="CloudGrid"):
        CR.plane_sums(xyz, e, e, xyz, nrm, g.border)
    base = dict(cloud_xyz=xyz, reference_xyz=xyz, border=g.border, max_dists=[1.0])
    for kw, msg in ((dict(metric="surface"), "metric"), (dict(metric="plane"), "one of the two"),
                    (dict(metric="plane", reference_normals=nrm, normal_radius=1.0), "one of the two"),
                    (dict(reference_normals=nrm), "belong to"), (dict(normal_radius=1.0), "belong to"),
                    (dict(metric="plane", normal_radius=0.0), "normal_radius"), (dict(metric="plane", normal_radius=1e-9), "2\\^21")):
        with pytest.raises(ValueError, match=msg):
            CR.register(**dict(base, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.register(**dict(base, metric="plane", normal_radius=1.0))


def test_the_command_line_knows_the_metric(capsys, tmp_path):
    base = ["--cloud", str(tmp_path / "a.ply"), "--reference", str(tmp_path / "b.ply"), "--border=0,4,0,4,0,4", "--max_dist=1.0"]
    for extra, msg in ((["--metric", "surface"], "invalid choice"), (["--normal_radius=1.0"], "belong to --metric plane"),
                       (["--z_down"], "belong to --metric plane"), (["--metric", "plane", "--normal_radius=0"], "normal_radius")):
        with pytest.raises(SystemExit):
            CR.main(base + extra)
        assert msg in capsys.readouterr().err, extra
