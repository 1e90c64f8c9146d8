"""Mesh decimation without a GPU: a numpy restatement of the rule of deep3d_aerial_amd/mesh.py (face incidence,
vertex quadrics, candidates with target / cost / validity / key, the K smallest keys, claims, winners, the mesh after a round),
checked on hand cases and for the properties the rule promises; the settings and the new flags of predict and of the mesh
command line; the new entry points refusing null pointers, bad sizes and short scratch before any launch.
tests/test_mesh_decimate_gpu.py holds the kernels to this restatement bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import test_mesh_clean as C
from deep3d_aerial_amd import _lib, mesh

HASH = 2654435761
I64_MAX = np.iinfo(np.int64).max


# ----------------------------------------------------------------------------------------
# the numpy restatement (fp64, one operation per numpy call: nothing is contracted)
# ----------------------------------------------------------------------------------------
def incidence_numpy(n, faces):
    """(face_offset [n+1] int32, face_index [3m] int32): the faces at every vertex in increasing face index."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    foff = np.zeros(n + 1, np.int32)
    foff[1:] = np.cumsum(np.bincount(flat, minlength=n))
    return foff, (order // 3).astype(np.int32)


def _normal(p0, p1, p2):
    u, w = p1 - p0, p2 - p0
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def face_quadrics_numpy(vertices, faces):
    p = np.asarray(vertices, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    p0 = p[:, 0]
    nrm = _normal(p0, p[:, 1], p[:, 2])
    ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    ok = ln > 0
    with np.errstate(all="ignore"):
        a, b, c = nrm[:, 0] / ln, nrm[:, 1] / ln, nrm[:, 2] / ln
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        w = ln * 0.5
        q = np.stack([w * (a * a), w * (a * b), w * (a * c), w * (a * d), w * (b * b), w * (b * c), w * (b * d), w * (c * c), w * (c * d),
                      w * (d * d)], 1)
    q[~ok] = 0.0   # adding +0 to a sum that started at +0 changes nothing
    return q


def vertex_quadrics_numpy(vertices, faces, foff, finc):
    n = len(vertices)
    fq = face_quadrics_numpy(vertices, faces)
    Q = np.zeros((n, 10), np.float64)
    deg = np.diff(foff.astype(np.int64))
    for k in range(int(deg.max()) if n else 0):
        idx = np.nonzero(deg > k)[0]
        Q[idx] = Q[idx] + fq[finc[foff[idx].astype(np.int64) + k]]
    return Q


def edges_numpy(offset, nbr):
    """[E,2]: the undirected edges a < b in lexicographic order."""
    n = len(offset) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(offset))
    up = nbr.astype(np.int64) > src
    return np.stack([src[up], nbr.astype(np.int64)[up]], 1)


def _expand(start, length):
    """owner and position of every entry of the rows (start, length)."""
    length = length.astype(np.int64)
    owner = np.repeat(np.arange(len(start), dtype=np.int64), length)
    first = np.cumsum(length) - length
    pos = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(first, length) + np.repeat(start.astype(np.int64), length)
    return owner, pos


def _eval(q, x):
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    r0 = ((q[:, 0] * X + q[:, 1] * Y) + q[:, 2] * Z) + q[:, 3]
    r1 = ((q[:, 1] * X + q[:, 4] * Y) + q[:, 5] * Z) + q[:, 6]
    r2 = ((q[:, 2] * X + q[:, 5] * Y) + q[:, 7] * Z) + q[:, 8]
    r3 = ((q[:, 3] * X + q[:, 6] * Y) + q[:, 8] * Z) + q[:, 9]
    return ((X * r0 + Y * r1) + Z * r2) + r3


def _cost(q, x):
    with np.errstate(all="ignore"):
        c = _eval(q, x)
    return np.where(c > 0, c, 0.0)


def minimiser_numpy(q):
    """(s [E,3], det [E]) by the Cramer's rule written out in mesh.py."""
    with np.errstate(all="ignore"):
        r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
        c00 = q[:, 4] * q[:, 7] - q[:, 5] * q[:, 5]
        c01 = q[:, 1] * q[:, 7] - q[:, 5] * q[:, 2]
        c02 = q[:, 1] * q[:, 5] - q[:, 4] * q[:, 2]
        det = (q[:, 0] * c00 - q[:, 1] * c01) + q[:, 2] * c02
        m0 = r1 * q[:, 7] - q[:, 5] * r2
        m1 = r1 * q[:, 5] - q[:, 4] * r2
        m2 = q[:, 1] * r2 - r1 * q[:, 2]
        sx = ((r0 * c00 - q[:, 1] * m0) + q[:, 2] * m1) / det
        sy = ((q[:, 0] * m0 - r0 * c01) + q[:, 2] * m2) / det
        sz = ((-(q[:, 0] * m1) - q[:, 1] * m2) + r0 * c02) / det
    return np.stack([sx, sy, sz], 1), det


def candidates_numpy(vertices, faces, offset, nbr, fixed, foff, finc, Q, edges):
    """(target [E,3] fp32, cost [E] fp32, key [E] int64; -1: not valid)."""
    v64 = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    n, E = len(v64), len(edges)
    ea, eb = edges[:, 0], edges[:, 1]
    fa, fb = fixed[ea] != 0, fixed[eb] != 0
    cand = ~(fa & fb)
    q = Q[ea] + Q[eb]
    xa, xb = v64[ea], v64[eb]
    mid = 0.5 * (xa + xb)
    d = xb - xa
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    s, det = minimiser_numpy(q)
    with np.errstate(all="ignore"):
        ds = s - mid
        dist2 = (ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]
        use_s = np.isfinite(det) & (det != 0) & (dist2 <= len2)
    x, best = xa.copy(), _cost(q, xa)
    cb = _cost(q, xb)
    sel = cb < best
    x[sel], best[sel] = xb[sel], cb[sel]
    cm = _cost(q, mid)
    sel = cm < best
    x[sel] = mid[sel]
    x = np.where(use_s[:, None], s, x)
    x = np.where(fa[:, None], xa, np.where(fb[:, None], xb, x))
    with np.errstate(all="ignore"):
        target = x.astype(np.float32)
        cost = _cost(q, x).astype(np.float32)
    # (i) link condition, (ii) degree
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(offset))
    codes = src * n + nbr.astype(np.int64)   # sorted: the CSR rows are
    deg = np.diff(offset)
    owner, pos = _expand(offset[ea], deg[ea])
    query = eb[owner] * n + nbr[pos].astype(np.int64)
    at = np.minimum(np.searchsorted(codes, query), max(len(codes) - 1, 0))
    found = (codes[at] == query) if len(codes) else np.zeros(0, bool)
    shared = np.bincount(owner, weights=found, minlength=E).astype(np.int64)
    valid = cand & (shared == 2) & (deg[ea] + deg[eb] - 4 >= 3)
    # (iii) flips at the fp32 target
    t64 = target.astype(np.float64)
    fdeg = np.diff(foff.astype(np.int64))
    for row, other in ((ea, eb), (eb, ea)):
        owner, pos = _expand(foff[row], fdeg[row])
        tri = f[finc[pos]]
        has_other = (tri == other[owner][:, None]).any(1)
        p = v64[tri]
        n0 = _normal(p[:, 0], p[:, 1], p[:, 2])
        p = np.where((tri == row[owner][:, None])[:, :, None], t64[owner][:, None, :], p)
        with np.errstate(all="ignore"):
            n1 = _normal(p[:, 0], p[:, 1], p[:, 2])
            dot = (n0[:, 0] * n1[:, 0] + n0[:, 1] * n1[:, 1]) + n0[:, 2] * n1[:, 2]
        bad = ~has_other & ~(dot > 0)
        valid &= np.bincount(owner, weights=bad, minlength=E) == 0
    target[~cand] = 0
    cost[~cand] = 0
    h = (np.arange(E, dtype=np.uint64) * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)
    key = ((cost.view(np.uint32).astype(np.uint64) << np.uint64(32)) | h).astype(np.int64)
    return target, cost, np.where(valid, key, -1)


def decimate_round_numpy(vertices, faces, target_faces):
    """One round: a dict with every pass's result and the mesh after it ("vertices", "faces", "winners")."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    n, m = len(v), len(f)
    K = max(0, -(-(m - int(target_faces)) // 2))
    offset, nbr, fixed = C.adjacency_numpy(n, f)
    foff, finc = incidence_numpy(n, f)
    Q = vertex_quadrics_numpy(v, f, foff, finc)
    edges = edges_numpy(offset, nbr)
    target, cost, key = candidates_numpy(v, f, offset, nbr, fixed, foff, finc, Q, edges)
    good = np.sort(key[key >= 0])
    thr = int(good[min(K, len(good)) - 1]) if K > 0 and len(good) else -1
    el = np.nonzero((key >= 0) & (key <= thr))[0]
    ea, eb = edges[el, 0], edges[el, 1]
    deg = np.diff(offset)
    oa, pa = _expand(offset[ea], deg[ea])
    ob, pb = _expand(offset[eb], deg[eb])
    who = np.concatenate([np.arange(len(el)), np.arange(len(el)), oa, ob]).astype(np.int64)
    where = np.concatenate([ea, eb, nbr[pa].astype(np.int64), nbr[pb].astype(np.int64)])
    claim = np.full(n, I64_MAX, np.int64)
    np.minimum.at(claim, where, key[el][who])
    lost = np.bincount(who, weights=claim[where] != key[el][who], minlength=len(el)) > 0
    win = np.zeros(len(edges), np.uint8)
    win[el[~lost]] = 1
    out = {"face_offset": foff, "face_index": finc, "quadric": Q, "offset": offset, "nbr": nbr, "fixed": fixed, "edges": edges.astype(np.int32),
           "target": target, "cost": cost, "key": key, "threshold": thr, "claim": claim, "win": win, "eligible": K,
           "winners": int(win.sum()), "vertices": v, "faces": f}
    if out["winners"] == 0:
        return out
    w = np.nonzero(win)[0]
    keep_b = (fixed[edges[w, 1]] != 0) & (fixed[edges[w, 0]] == 0)
    s, r = np.where(keep_b, edges[w, 1], edges[w, 0]), np.where(keep_b, edges[w, 0], edges[w, 1])
    v2 = v.copy()
    v2[s] = target[w]
    remap = np.arange(n, dtype=np.int64)
    remap[r] = s
    f2 = remap[f]
    kf = f2[(f2[:, 0] != f2[:, 1]) & (f2[:, 1] != f2[:, 2]) & (f2[:, 2] != f2[:, 0])]
    used = np.zeros(n, bool)
    used[kf.ravel()] = True
    renum = np.cumsum(used) - 1
    out.update(vertices=v2[used], faces=renum[kf].astype(np.int32).reshape(-1, 3))
    return out


def decimate_numpy(vertices, faces, ratio=1.0, target_faces=0, max_rounds=mesh.DEFAULT_DECIMATE_MAX_ROUNDS, each_round=None):
    """(vertices, faces, info) as mesh.decimate; each_round(round dict) is called after every round."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    m0 = len(f)
    goal = target_faces if target_faces > 0 else int(math.ceil(ratio * m0))
    info = {"target_faces": goal, "rounds": 0, "collapses": [], "faces_in": m0, "stalled": False, "hit_max_rounds": False}
    while len(f) > goal and not ((ratio == 1.0 and target_faces == 0)):
        if info["rounds"] >= max_rounds:
            info["hit_max_rounds"] = True
            break
        r = decimate_round_numpy(v, f, goal)
        if each_round is not None:
            each_round(r)
        v, f = r["vertices"], r["faces"]
        info["rounds"] += 1
        info["collapses"].append(r["winners"])
        if r["winners"] == 0:
            info["stalled"] = True
            break
    info.update(faces_out=len(f), vertices_out=len(v))
    return v, f, info


# ----------------------------------------------------------------------------------------
# cases (shared with the GPU tests)
# ----------------------------------------------------------------------------------------
def grid_mesh(k=24, noise=0.0, seed=0, kx=None):
    """A kx x k vertex grid in z = 0 (cell 1), two triangles per cell; noise: fp32 uniform noise on every coordinate of the
    interior vertices, in cells."""
    kx = k if kx is None else kx
    i, j = np.meshgrid(np.arange(k), np.arange(kx), indexing="ij")
    v = np.stack([j.ravel(), i.ravel(), np.zeros(k * kx)], 1).astype(np.float32)
    if noise:
        inner = ((i > 0) & (i < k - 1) & (j > 0) & (j < kx - 1)).ravel()
        v[inner] += (np.random.default_rng(seed).uniform(-noise, noise, (int(inner.sum()), 3))).astype(np.float32)
    a = (i[:-1, :-1] * kx + j[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + kx], 1), np.stack([a + 1, a + kx + 1, a + kx], 1)]).astype(np.int32)
    return v, f


def sphere_mesh(nlat=16, nlon=24, radius=3.0):
    """A closed latitude / longitude sphere with two poles."""
    v = [[0, 0, radius]]
    for a in range(1, nlat):
        th = np.pi * a / nlat
        for b in range(nlon):
            ph = 2 * np.pi * b / nlon
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    v.append([0, 0, -radius])
    ring = lambda a, b: 1 + (a - 1) * nlon + b % nlon
    f = [[0, ring(1, b), ring(1, b + 1)] for b in range(nlon)]
    for a in range(1, nlat - 1):
        for b in range(nlon):
            f += [[ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)], [ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)]]
    f += [[len(v) - 1, ring(nlat - 1, b + 1), ring(nlat - 1, b)] for b in range(nlon)]
    return np.array(v, np.float32), np.array(f, np.int32)


def cone_mesh(k=1500):
    """An apex of k faces over a free ring (radius 1), and a boundary ring (radius 2) around it."""
    ang = np.arange(k) * 2 * np.pi / k
    ring = lambda r, z: np.stack([r * np.cos(ang), r * np.sin(ang), np.full(k, z)], 1)
    v = np.concatenate([[[0, 0, 1.0]], ring(1.0, 0.5), ring(2.0, 0.0)]).astype(np.float32)
    i = np.arange(k)
    nx = (i + 1) % k
    f = np.concatenate([np.stack([np.zeros(k, int), 1 + i, 1 + nx], 1), np.stack([1 + i, 1 + k + i, 1 + k + nx], 1),
                        np.stack([1 + i, 1 + k + nx, 1 + nx], 1)]).astype(np.int32)
    return v, f


def two_free_mesh():
    """A 4 x 3 vertex grid: exactly two free vertices (5 and 6), adjacent to each other, so every candidate's neighbourhood
    holds both and no two candidates are independent."""
    v, f = grid_mesh(3, kx=4)
    v[5, 2], v[6, 2] = 0.25, 0.125
    return v, f


def _areas(v, f):
    p = v.astype(np.float64)[f.astype(np.int64)]
    nrm = _normal(p[:, 0], p[:, 1], p[:, 2])
    return 0.5 * np.sqrt((nrm * nrm).sum(1))


def _pos_edges(v, lo, hi, sel):
    key = lambda i: v[i].tobytes()
    return sorted(tuple(sorted((key(a), key(b)))) for a, b in zip(lo[sel].tolist(), hi[sel].tolist()))


def check_properties(v0, f0, v1, f1, adjacency=C.adjacency_numpy):
    """What the rule promises on a manifold mesh: no new boundary or non-manifold edge and the same boundary edges, the fixed
    vertices where they were, the same Euler characteristic and component count, no face of zero area."""
    lo0, hi0, c0 = C.edges_numpy(f0)
    lo1, hi1, c1 = C.edges_numpy(f1)
    assert _pos_edges(v0, lo0, hi0, c0 != 2) == _pos_edges(v1, lo1, hi1, c1 != 2)
    fx0, fx1 = adjacency(len(v0), f0)[2], adjacency(len(v1), f1)[2]
    assert sorted(v0[fx0 != 0].view(np.int32).tolist()) == sorted(v1[fx1 != 0].view(np.int32).tolist())
    euler = lambda f, lo: len(np.unique(f)) - len(lo) + len(f)
    assert euler(f0, lo0) == euler(f1, lo1)
    assert len(np.unique(f1)) == len(v1)
    assert len(np.unique(C.components_numpy(len(v0), f0))) == len(np.unique(C.components_numpy(len(v1), f1)))
    assert (_areas(v1, f1) > 0).all()
    assert ((f1[:, 0] != f1[:, 1]) & (f1[:, 1] != f1[:, 2]) & (f1[:, 2] != f1[:, 0])).all()


# ----------------------------------------------------------------------------------------
# hand cases
# ----------------------------------------------------------------------------------------
def test_incidence_and_quadrics_of_a_fan():
    v, f = C.HAND["fan"]
    foff, finc = incidence_numpy(7, f)
    assert foff.tolist() == [0, 6, 8, 10, 12, 14, 16, 18] and finc[:6].tolist() == [0, 1, 2, 3, 4, 5] and finc[6:8].tolist() == [0, 5]
    Q = vertex_quadrics_numpy(v, f, foff, finc)
    fq = face_quadrics_numpy(v, f)
    want = np.zeros(10)
    for k in range(6):
        want = want + fq[k]
    assert np.array_equal(Q[0], want) and np.array_equal(Q[1], (np.zeros(10) + fq[0]) + fq[5])
    # a face quadric is area * (distance to its plane)^2
    p = v.astype(np.float64)
    assert abs(_eval(fq[:1], p[None, 0])[0]) < 1e-15 and abs(_eval(fq[:1], p[None, 1])[0]) < 1e-15
    nrm = _normal(p[None, 0], p[None, 1], p[None, 2])[0]
    off = p[0] + 0.5 * nrm / np.linalg.norm(nrm)
    assert abs(_eval(fq[:1], off[None])[0] - _areas(v, f)[0] * 0.25) < 1e-12
    zero = face_quadrics_numpy(np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), np.int32([[0, 1, 2]]))
    assert np.array_equal(zero, np.zeros((1, 10)))   # a face without area contributes nothing


def test_cramer_minimiser_is_the_corner_of_three_planes():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A = rng.standard_normal((3, 3))
        A /= np.linalg.norm(A, axis=1, keepdims=True)
        x0 = rng.standard_normal(3) * 10
        d = -A @ x0
        q = np.zeros(10)
        for (a, b, c), dd in zip(A, d):
            q += np.array([a * a, a * b, a * c, a * dd, b * b, b * c, b * dd, c * c, c * dd, dd * dd])
        s, det = minimiser_numpy(q[None])
        assert det[0] != 0 and np.allclose(s[0], np.linalg.solve(A, -d), atol=1e-9 / abs(det[0]))
        assert abs(_eval(q[None], x0[None])[0]) < 1e-9


def test_closed_tetrahedron_comes_back_unchanged_and_stalled():
    v, f = C.HAND["tetrahedron"]
    r = decimate_round_numpy(v, f, 2)
    assert len(r["edges"]) == 6 and (r["key"] == -1).all() and r["winners"] == 0   # rule 5 (ii): 3 + 3 - 4 < 3
    V, F, info = decimate_numpy(v, f, ratio=0.5)
    assert np.array_equal(V, v) and np.array_equal(F, f) and info["stalled"] and info["rounds"] == 1 and info["faces_out"] == 4


def test_two_adjacent_cheapest_edges_only_the_smaller_key_wins():
    v, f = two_free_mesh()
    offset, nbr, fixed = C.adjacency_numpy(len(v), f)
    assert np.nonzero(fixed == 0)[0].tolist() == [5, 6] and 6 in nbr[offset[5]:offset[6]].tolist()
    r = decimate_round_numpy(v, f, len(f) - 4)   # K = 2: the two cheapest valid candidates are eligible
    key = r["key"]
    el = np.nonzero((key >= 0) & (key <= r["threshold"]))[0]
    assert len(el) == 2 and r["eligible"] == 2
    assert r["winners"] == 1 and r["win"][el[np.argmin(key[el])]] == 1 and len(r["faces"]) == len(f) - 2
    check_properties(v, f, r["vertices"], r["faces"])


def test_planar_grid_stays_planar_keeps_its_area_and_reaches_the_target():
    v, f = grid_mesh(24)
    assert len(f) == 1058
    V, F, info = decimate_numpy(v, f, ratio=0.25)
    assert info["target_faces"] == 265 and not info["stalled"] and not info["hit_max_rounds"]
    assert len(F) in (264, 265) and info["rounds"] < 200
    assert (V[:, 2].view(np.int32) == 0).all()
    assert abs(_areas(V, F).sum() - 529.0) < 1e-9
    check_properties(v, f, V, F)
    lo, hi, cnt = C.edges_numpy(F)
    assert int((cnt == 1).sum()) == 92 and len(V) - len(lo) + len(F) == 1
    print("planar grid rounds", info["rounds"], info["collapses"])


def test_noisy_grid_sphere_and_cone_keep_their_topology():
    for name, (v, f), kw in (("noisy", grid_mesh(24, 0.02, 3), {"ratio": 0.25}), ("sphere", sphere_mesh(), {"target_faces": 200}),
                             ("cone", cone_mesh(300), {"ratio": 0.5})):
        V, F, info = decimate_numpy(v, f, **kw)
        check_properties(v, f, V, F)
        assert info["stalled"] or len(F) in (info["target_faces"], info["target_faces"] - 1), (name, info)
        assert len(F) < len(f)
        print(name, info["rounds"], info["faces_out"], info["stalled"])
        if name == "sphere":
            assert not info["stalled"] and len(F) == 200
            r = np.linalg.norm(V.astype(np.float64), axis=1)
            assert r.min() > 2.5 and r.max() < 3.3   # still a sphere of radius 3


def test_off_returns_the_input_and_max_rounds_is_reported():
    v, f = grid_mesh(8)
    V, F, info = decimate_numpy(v, f)
    assert np.array_equal(V, v) and np.array_equal(F, f) and info["rounds"] == 0
    V, F, info = decimate_numpy(v, f, ratio=0.3, max_rounds=2)
    assert info["hit_max_rounds"] and info["rounds"] == 2 and not info["stalled"] and len(F) > info["target_faces"]


def test_keys_order_by_cost_then_hash_and_winners_are_independent():
    v, f = grid_mesh(12, 0.05, 1)
    r = decimate_round_numpy(v, f, 100)
    ok = r["key"] >= 0
    assert ok.sum() > 50
    assert np.array_equal(r["key"][ok] >> 32, r["cost"][ok].view(np.int32).astype(np.int64))
    assert np.array_equal(r["key"][ok] & 0xFFFFFFFF, (np.nonzero(ok)[0] * HASH) % (1 << 32))
    h = (np.arange(1 << 16, dtype=np.uint64) * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)
    assert len(np.unique(h)) == 1 << 16 and mesh.DECIMATE_HASH == HASH and HASH % 2 == 1   # an odd multiplier: a bijection
    seen = np.zeros(len(v), int)
    for e in np.nonzero(r["win"])[0]:
        a, b = r["edges"][e]
        ws = {int(a), int(b)} | set(r["nbr"][r["offset"][a]:r["offset"][a + 1]].tolist()) | set(r["nbr"][r["offset"][b]:r["offset"][b + 1]].tolist())
        seen[list(ws)] += 1
    assert seen.max() == 1 and r["winners"] >= 2   # no vertex lies in two winners' neighbourhoods
    assert r["win"][np.nonzero(ok)[0][np.argmin(r["key"][ok])]] == 1   # the smallest key always wins


# ----------------------------------------------------------------------------------------
# settings and command lines
# ----------------------------------------------------------------------------------------
def test_decimate_settings():
    assert mesh.check_decimate_settings() == (1.0, 0, mesh.DEFAULT_DECIMATE_MAX_ROUNDS)
    assert mesh.check_decimate_settings(0.25, 0, 50) == (0.25, 0, 50)
    assert mesh.check_decimate_settings(1.0, 1000) == (1.0, 1000, mesh.DEFAULT_DECIMATE_MAX_ROUNDS)
    assert mesh.DEFAULT_DECIMATE_MAX_ROUNDS >= 500
    for kw, what in (({"ratio": 0}, "ratio"), ({"ratio": 1.5}, "ratio"), ({"ratio": float("nan")}, "ratio"), ({"target_faces": -1}, "target_faces"),
                     ({"target_faces": 2.5}, "target_faces"), ({"ratio": 0.5, "target_faces": 10}, "one of them"), ({"max_rounds": 0}, "max_rounds")):
        with pytest.raises(ValueError, match=what):
            mesh.check_decimate_settings(**kw)
    assert not mesh.decimate_requested({"path": "x", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1})   # older settings dicts: off
    assert mesh.decimate_requested({"decimate": 0.5}) and mesh.decimate_requested({"target_faces": 100})
    assert not mesh.decimate_requested({"decimate": 1.0, "target_faces": 0})
    assert mesh.check_clean_settings() == (0, 0.0, 0, 0.5)   # the clean settings keep their own tuple


def test_predict_and_mesh_command_line_flags(capsys):
    from deep3d_aerial_amd import predict

    base = ["--model", "casmvsnet", "--loadckpt", "x.ckpt", "--data_folder", "d", "--output_folder", "o", "--fuse", "--mesh", "m.ply",
            "--mesh_border", "0,1,0,1,0,1", "--mesh_voxel", "0.1"]
    s = predict._mesh_settings(predict.parse_args(base))
    assert (s["decimate"], s["target_faces"], s["decimate_max_rounds"]) == (1.0, 0, mesh.DEFAULT_DECIMATE_MAX_ROUNDS)
    assert not mesh.decimate_requested(s)
    s = predict._mesh_settings(predict.parse_args(base + ["--mesh_decimate", "0.25", "--mesh_decimate_max_rounds", "40"]))
    assert mesh.decimate_settings(s) == (0.25, 0, 40) and mesh.decimate_requested(s)
    s = predict._mesh_settings(predict.parse_args(base + ["--mesh_target_faces", "5000"]))
    assert mesh.decimate_settings(s) == (1.0, 5000, mesh.DEFAULT_DECIMATE_MAX_ROUNDS) and mesh.decimate_requested(s)
    for bad, what in ((["--mesh_decimate", "0"], "ratio"), (["--mesh_decimate", "1.2"], "ratio"), (["--mesh_target_faces", "-4"], "target_faces"),
                      (["--mesh_decimate", "0.5", "--mesh_target_faces", "10"], "one of them"), (["--mesh_decimate_max_rounds", "0"], "max_rounds")):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
        assert what in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--out", "o.ply", "--decimate", "0.5", "--target_faces", "10"])
    assert "one of them" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--mvs", "x", "--out", "o.ply", "--border", "0,1,0,1,0,1", "--voxel", "0.1", "--decimate", "-1"])
    assert "ratio" in capsys.readouterr().err


def test_new_entry_points_refuse_null_pointers_bad_sizes_and_short_scratch_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(8)
    big = 1 << 20
    assert lib.d3d_mesh_decimate_incidence(None, 0, 0, None, 0, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_incidence(p, -1, 4, p, big, p, p, None) == -1
    assert lib.d3d_mesh_decimate_incidence(p, 1 << 29, 4, p, big, p, p, None) == -1   # 6 m >= 2^31
    assert lib.d3d_mesh_decimate_incidence(p, 4, 4, p, 16, p, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_quadrics(None, 4, None, 4, None, None, None, None) == -1
    assert lib.d3d_mesh_decimate_quadrics(p, 1 << 31, p, 4, p, p, p, None) == -1
    assert lib.d3d_mesh_decimate_edges(None, None, 0, None, 0, 0, None, None, None) == -1
    assert lib.d3d_mesh_decimate_edges(p, p, 4, p, 16, 12, p, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_edges(p, p, 4, p, big, 1 << 31, p, p, None) == -1   # more than 2^31 - 1 edges
    assert b"max_edges" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_candidates(None, 0, None, 0, None, None, None, None, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.d3d_mesh_decimate_candidates(p, 4, p, -2, p, p, p, p, p, p, p, p, 12, p, p, p, None) == -1
    assert lib.d3d_mesh_decimate_candidates(p, 4, p, 4, p, p, p, p, p, p, p, p, -1, p, p, p, None) == -1
    assert lib.d3d_mesh_decimate_select(None, 0, 0, None, 0, None, None) == -1
    assert lib.d3d_mesh_decimate_select(p, 12, -1, p, big, p, None) == -1
    assert b"k=" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_select(p, 12, 3, p, 8, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_claim(None, None, 0, None, None, None, 0, None, None, None, None) == -1
    assert lib.d3d_mesh_decimate_claim(p, p, -1, p, p, p, 12, p, p, p, None) == -1
    assert lib.d3d_mesh_decimate_apply(None, 0, None, None, None, None, None, None, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.d3d_mesh_decimate_apply(p, 4, p, p, p, p, p, p, p, 12, p, p, p, p, p, p, None) == -1   # out_vertices aliases the input
    assert b"distinct" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_faces(None, 0, 0, None, None, 0, None, None, None, None) == -1
    assert lib.d3d_mesh_decimate_faces(p, 4, 4, p, p, 16, p, p, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_decimate_incidence_scratch_bytes(-1, 0) == 0 and lib.d3d_mesh_decimate_incidence_scratch_bytes(10, 1 << 29) == 0
    assert lib.d3d_mesh_decimate_incidence_scratch_bytes(10, 10) >= 4 * 60
    assert lib.d3d_mesh_decimate_edges_scratch_bytes(-1) == 0 and lib.d3d_mesh_decimate_edges_scratch_bytes(10) >= 80
    assert lib.d3d_mesh_decimate_select_scratch_bytes() >= 1024 + 16
    assert lib.d3d_mesh_decimate_faces_scratch_bytes(-1) == 0 and lib.d3d_mesh_decimate_faces_scratch_bytes(10) >= 80


def test_decimate_refuses_cpu_tensors_and_bad_settings():
    import torch

    v, f = grid_mesh(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.decimate(torch.from_numpy(v), torch.from_numpy(f), ratio=0.5)
    with pytest.raises(ValueError, match="one of them"):
        mesh.decimate(torch.from_numpy(v), torch.from_numpy(f), ratio=0.5, target_faces=3)
