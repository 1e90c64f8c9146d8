"""A mesh to flip and the rule of deep3d_aerial_amd/flip.py restated in numpy from its text, for tests/test_mesh_flip.py and
tests/test_mesh_flip_gpu.py.

The restatement (flip_round_numpy, flip_numpy) works in Python floats, fp64 one operation at a time with nothing contracted, every
dot product and squared length summed (x x + y y) + z z, and keeps the keys as Python integers until the claim is decided.

The scene: MAX_ANGLE is 30 degrees.  The pieces are disjoint and placed apart, and `cases` names them by their vertex indices.
The hand-built ones have dyadic coordinates.  A "quad" is the pair (a, b, c), (b, a, d) around the edge a-b with a wing triangle
(a, c, ea) and (b, d, eb) at each end, which gives a and b a fourth neighbour:
* "cap": c lies 1/8 above the middle of a-b, d one unit below: the flip to c-d gains, and it happens;
* "zero": the same with c on a-b, three collinear vertices: the old normal of (a, b, c) is zero, and the flip happens;
* "regular": a square cut by a diagonal: the other diagonal gives the same qualities, no strict gain: it stays;
* "boundary": a lone triangle, every edge with one face; "three": an edge with three faces; "inconsistent": two faces that both hold
  a->b: the pair test refuses them;
* "exists": the cap with a triangle (c, d, p) standing on it, so the edge c-d exists already (test 4.1);
* "degree": the cap without the wing at a, which has three neighbours (test 4.2);
* "roof": a ridge a-b whose sides meet at 45 degrees, steeper than the guard, and whose flip would otherwise gain (test 4.3);
* "concave": a planar quad whose corner b is reflex: the flip gains in quality and (b, c, d) turns over (test 4.4 alone);
* "shared": two caps in a row, the first one's b the second one's a.  The first is the worse: it wins the shared vertex in round
  1, and the second flips in round 2;
* "fan": 40 faces around one vertex (the smaller index of every spoke, so each spoke walks a face row of 40) inside a ring of 40
  more, the centre a little off the middle;
* "unreferenced": a vertex no face uses;
* "grid": GRID_N x GRID_N vertices with unit spacing, jittered by +-JITTER in x and y, z noise of sigma Z_SIGMA, a random diagonal
  per cell: about 4600 edges, many workgroups of 256 with a partial last one, hundreds of candidates whose claims collide.
SEED was chosen on the CPU, by the restatement alone, among the first seeds for which round 1 has more than 512 candidates and
fewer winners than candidates, and the chain ends with a round of no candidates before round 16: tests/test_mesh_flip.py asserts
all three."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_mesh_clean as C  # noqa: E402
import test_mesh_decimate as D  # noqa: E402

HASH = 2654435761
I64_MAX = (1 << 63) - 1
TESTS = ("pair", "new_edge", "degree", "guard", "turn", "gain")
MAX_ANGLE = 30.0
ROUNDS = 16
GRID_N = 40
JITTER = 0.45
Z_SIGMA = 0.05
FAN = 40
FAN_CENTRE = (0.25, 0.125)   # in a rim of radius 2
SEED = 0


# ----------------------------------------------------------------------------------------
# the rule in numpy
# ----------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _d2(p, q):
    dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
    return (dx * dx + dy * dy) + dz * dz


def _normal(p0, p1, p2):
    ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    vx, vy, vz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return (uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx)


def quality(X, i, j, k):
    """Rule 5's Q of the triangle with the vertex indices i, j, k (any order) at the positions X."""
    p0, p1, p2 = (X[v] for v in sorted((i, j, k)))
    n = _normal(p0, p1, p2)
    s = (_d2(p0, p1) + _d2(p1, p2)) + _d2(p2, p0)
    return 0.0 if s == 0.0 else _dot(n, n) / (s * s)


def _min(x, y):
    return x if x < y else y


def cos2(max_angle):
    c = math.cos(math.radians(float(max_angle)))
    return c * c


def qualities(V, F):
    """Q of every face, ascending: the vector rule 5 says grows lexicographically with every flip."""
    X = np.asarray(V, np.float32).astype(np.float64).tolist()
    return sorted(quality(X, *f) for f in np.asarray(F).tolist())


def flip_round_numpy(V, F, max_angle=MAX_ANGLE):
    """One round (rules 2-8).  The dict of every pass: offset, nbr, fixed, face_offset, face_index, edges, key, opp, passed (per
    test name a bool [E]: "pair" for rule 3, then every test of rules 4 and 5 judged by itself on the edges that have a pair),
    claim, win, candidates, winners, and the mesh after it (vertices, faces)."""
    V, F = np.asarray(V, np.float32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    n = len(V)
    offset, nbr, fixed = C.adjacency_numpy(n, F)
    foff, finc = D.incidence_numpy(n, F)
    E = D.edges_numpy(offset, nbr).astype(np.int32).reshape(-1, 2)
    X = V.astype(np.float64).tolist()
    tris = F.tolist()
    rows = [set(nbr[offset[v]:offset[v + 1]].tolist()) for v in range(n)]
    c2 = cos2(max_angle)
    keys = [-1] * len(E)
    opp = np.zeros((len(E), 4), np.int32)
    passed = {k: np.zeros(len(E), bool) for k in TESTS}
    for e, (a, b) in enumerate(E.tolist()):
        ab, ba = [], []
        for f in finc[foff[a]:foff[a + 1]].tolist():
            tri = tris[f]
            if b not in tri:
                continue
            i = tri.index(a)
            if tri[(i + 1) % 3] == b:
                ab.append((f, tri[(i + 2) % 3]))
            else:
                ba.append((f, tri[(i + 1) % 3]))
        if len(ab) != 1 or len(ba) != 1 or ab[0][1] == ba[0][1]:
            continue
        (f_ab, c), (f_ba, d) = ab[0], ba[0]
        xa, xb, xc, xd = X[a], X[b], X[c], X[d]
        n1, n2 = _normal(xa, xb, xc), _normal(xb, xa, xd)
        dot = _dot(n1, n2)
        s = (n1[0] + n2[0], n1[1] + n2[1], n1[2] + n2[2])
        q_old = _min(quality(X, a, b, c), quality(X, b, a, d))
        q_new = _min(quality(X, a, d, c), quality(X, b, c, d))
        ok = {"pair": True, "new_edge": d not in rows[c], "degree": len(rows[a]) > 3 and len(rows[b]) > 3,
              "guard": dot >= 0.0 and dot * dot >= c2 * (_dot(n1, n1) * _dot(n2, n2)),
              "turn": _dot(_normal(xa, xd, xc), s) > 0.0 and _dot(_normal(xb, xc, xd), s) > 0.0, "gain": q_new > q_old}
        for k in TESTS:
            passed[k][e] = ok[k]
        if all(ok.values()):
            keys[e] = (int(np.float32(q_old).view(np.uint32)) << 32) | ((e * HASH) & 0xFFFFFFFF)
            opp[e] = (c, d, f_ab, f_ba)
    claim = [I64_MAX] * n
    for e, k in enumerate(keys):
        if k >= 0:
            for v in (int(E[e, 0]), int(E[e, 1]), int(opp[e, 0]), int(opp[e, 1])):
                claim[v] = min(claim[v], k)
    win = np.zeros(len(E), np.uint8)
    out = F.copy()
    for e, k in enumerate(keys):
        if k >= 0 and all(claim[v] == k for v in (int(E[e, 0]), int(E[e, 1]), int(opp[e, 0]), int(opp[e, 1]))):
            a, b, (c, d, f_ab, f_ba) = int(E[e, 0]), int(E[e, 1]), opp[e].tolist()
            win[e] = 1
            out[f_ab] = (a, d, c)
            out[f_ba] = (b, c, d)
    return {"offset": offset, "nbr": nbr, "fixed": fixed, "face_offset": foff, "face_index": finc, "edges": E, "key": np.array(keys, np.int64),
            "opp": opp, "passed": passed, "claim": np.array(claim, np.int64), "win": win, "candidates": sum(1 for k in keys if k >= 0),
            "winners": int(win.sum()), "vertices": V, "faces": out}


def flip_numpy(V, F, max_angle=MAX_ANGLE, rounds=ROUNDS, detail=None):
    """Rule 9: (vertices, faces, info) as flip.flip_edges; detail (a list) gets every round's dict."""
    V, F = np.asarray(V, np.float32).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3)
    info = {"edges": [], "candidates": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces": len(F)}
    for k in range(rounds if len(V) and len(F) else 0):
        r = flip_round_numpy(V, F, max_angle)
        if detail is not None:
            detail.append(r)
        info["rounds"] += 1
        info["edges"].append(len(r["edges"]))
        info["candidates"].append(r["candidates"])
        info["winners"].append(r["winners"])
        if r["winners"] == 0:
            break
        F = r["faces"]
        info["hit_max_rounds"] = k + 1 == rounds
    info["flips"] = sum(info["winners"])
    return V, F, info


# ----------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------
class _Builder(object):
    def __init__(self):
        self.V, self.F, self.cases = [], [], {}

    def vertices(self, pts, origin=(0.0, 0.0, 0.0)):
        first = len(self.V)
        origin = tuple(origin) + (0.0,) * (3 - len(origin))
        for p in pts:
            p = tuple(p) + (0.0,) * (3 - len(p))
            self.V.append([float(origin[i]) + float(p[i]) for i in range(3)])
        return list(range(first, len(self.V)))

    def faces(self, tris):
        self.F.extend([int(a), int(b), int(c)] for a, b, c in tris)


def _quad(B, origin, a, b, c, d, wing_a=True, wing_b=True):
    """The pair (a, b, c), (b, a, d) at the given points (2 or 3 coordinates), with the wings (a, c, ea), ea one unit above a,
    and (b, d, eb), eb one unit below b: the dict of the vertex indices."""
    ia, ib, ic, id_ = B.vertices([a, b, c, d], origin)
    B.faces([(ia, ib, ic), (ib, ia, id_)])
    out = {"a": ia, "b": ib, "c": ic, "d": id_}
    if wing_a:
        out["ea"], = B.vertices([(a[0], a[1] + 1.0)], origin)
        B.faces([(ia, ic, out["ea"])])
    if wing_b:
        out["eb"], = B.vertices([(b[0], b[1] - 1.0)], origin)
        B.faces([(ib, id_, out["eb"])])
    return out


def build(seed=SEED):
    """(V [n, 3] fp32, F [m, 3] int32, cases): cases names the crafted pieces by their vertex indices."""
    B = _Builder()
    A, Bb, Dn = (-1.0, 0.0), (1.0, 0.0), (0.0, -1.0)
    B.cases["cap"] = _quad(B, (0.0, 0.0), A, Bb, (0.0, 0.125), Dn)
    B.cases["zero"] = _quad(B, (8.0, 0.0), A, Bb, (0.0, 0.0), Dn)
    B.cases["regular"] = _quad(B, (16.0, 0.0), A, Bb, (0.0, 1.0), Dn)
    t = B.vertices([(0, 0), (1, 0), (0, 1)], (24.0, 0.0))
    B.faces([t])
    B.cases["boundary"] = tuple(t)
    a, b, c, d, e = B.vertices([A, Bb, (0, 1), Dn, (0, 0.5, 1)], (32.0, 0.0))
    B.faces([(a, b, c), (b, a, d), (a, b, e)])
    B.cases["three"] = {"a": a, "b": b, "c": c, "d": d, "e": e}
    a, b, c, d = B.vertices([A, Bb, (0, 1), Dn], (40.0, 0.0))
    B.faces([(a, b, c), (a, b, d)])
    B.cases["inconsistent"] = {"a": a, "b": b, "c": c, "d": d}
    q = _quad(B, (48.0, 0.0), A, Bb, (0.0, 0.125), Dn)
    q["p"], = B.vertices([(0.0, -0.5, 1.0)], (48.0, 0.0))
    B.faces([(q["c"], q["d"], q["p"])])
    B.cases["exists"] = q
    B.cases["degree"] = _quad(B, (56.0, 0.0), A, Bb, (0.0, 0.125), Dn, wing_a=False)
    B.cases["roof"] = _quad(B, (64.0, 0.0), A, Bb, (0.0, 0.25, 0.25), Dn)
    B.cases["concave"] = _quad(B, (72.0, 0.0), A, Bb, (3.0, 1.0), (3.0, -1.0))
    # two caps in a row: the first one's b is the second one's a
    a1, b1, c1, d1, b2, c2, d2, ea, eb = B.vertices([A, Bb, (0, 0.125), Dn, (3, 0), (2, 0.25), (2, -1), (-1, 1), (3, -1)], (84.0, 0.0))
    B.faces([(a1, b1, c1), (b1, a1, d1), (b1, b2, c2), (b2, b1, d2), (a1, c1, ea), (b2, d2, eb)])
    B.cases["shared"] = ({"a": a1, "b": b1, "c": c1, "d": d1}, {"a": b1, "b": b2, "c": c2, "d": d2})
    # the fan: the centre first, so that it is the smaller end of every spoke
    ang = 2.0 * np.pi * np.arange(FAN) / FAN
    centre, = B.vertices([FAN_CENTRE], (96.0, 0.0))
    rim = B.vertices([(2.0 * np.cos(t), 2.0 * np.sin(t)) for t in ang], (96.0, 0.0))
    ring = B.vertices([(3.0 * np.cos(t + np.pi / FAN), 3.0 * np.sin(t + np.pi / FAN)) for t in ang], (96.0, 0.0))
    B.faces([(centre, rim[i], rim[(i + 1) % FAN]) for i in range(FAN)])
    B.faces([(rim[i], ring[i], rim[(i + 1) % FAN]) for i in range(FAN)])
    B.cases["fan"] = (centre, rim, ring)
    B.cases["unreferenced"] = B.vertices([(104.0, 0.0, 1.0)])[0]
    # the jittered grid
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(GRID_N, dtype=np.float64), np.arange(GRID_N, dtype=np.float64))
    pts = np.stack([gx.ravel() + rng.uniform(-JITTER, JITTER, gx.size), 8.0 + gy.ravel() + rng.uniform(-JITTER, JITTER, gx.size),
                    rng.normal(0.0, Z_SIGMA, gx.size)], 1)
    grid = np.array(B.vertices(pts.tolist())).reshape(GRID_N, GRID_N)
    cut = rng.random((GRID_N - 1, GRID_N - 1)) < 0.5
    for j in range(GRID_N - 1):
        for i in range(GRID_N - 1):
            a, b, c, d = grid[j, i], grid[j, i + 1], grid[j + 1, i], grid[j + 1, i + 1]
            B.faces([(a, b, d), (a, d, c)] if cut[j, i] else [(a, b, c), (b, d, c)])
    B.cases["grid"] = grid
    return np.array(B.V, np.float64).astype(np.float32), np.array(B.F, np.int32), B.cases
