"""Helpers of tests/test_mesh_compare.py and tests/test_mesh_compare_gpu.py: the numpy restatement of the sampling rule of
deep3d_aerial_amd/mesh_compare.py, op by op in fp64, the restatements of the face error and of the two output
files, and the scenes the tests share."""
import struct

import numpy as np

N_MAX = 32768
NAN, INF = np.nan, np.inf


# ----------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------
def counts_numpy(vertices, faces, s):
    """(n [m] int64, clipped [m] bool): n_f of every face and whether it was cut down to N_MAX."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    s = np.float64(s)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]

    def edge2(a, b):
        d = a - b
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    with np.errstate(invalid="ignore", over="ignore"):
        L2 = np.maximum(np.maximum(edge2(A, B), edge2(B, C)), edge2(C, A))
        ok = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1) & np.isfinite(L2) & (L2 > 0)
        q = np.sqrt(np.where(ok, L2, 1.0)) / s
    clipped = ok & (q > N_MAX)
    n = np.where(q <= 1.0, 1.0, np.ceil(np.minimum(q, N_MAX)))
    return np.where(ok, n, 0).astype(np.int64), clipped


def isqrt_numpy(t):
    """floor(sqrt(t)) of non-negative integers, exactly."""
    t = np.asarray(t, np.int64)
    r = np.sqrt(t.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > t, r - 1, r)
    return np.where((r + 1) * (r + 1) <= t, r + 1, r)


def weights(n):
    """(p, q, w), each [n^2] int64: the integer weights of sample t = 0 .. n^2 - 1 of a face with n_f = n."""
    t = np.arange(n * n, dtype=np.int64)
    r = isqrt_numpy(t)
    c = t - r * r
    k = c >> 1
    odd = (c & 1) == 1
    p = np.where(odd, 3 * (n - r) - 1, 3 * (n - r) - 2)
    q = np.where(odd, 3 * k + 2, 3 * k + 1)
    w = np.where(odd, 3 * (r - k) - 1, 3 * (r - k) + 1)
    return p, q, w


def sample_numpy(vertices, faces, s, rounded=True):
    """(xyz [S,3], face [S] int32, offsets [m+1] int64) of the rule; xyz is float32, or the fp64 values before the last rounding
    with rounded=False.  A clipped face is an AssertionError: the tests never sample one."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n, clipped = counts_numpy(vertices, faces, s)
    assert not clipped.any()
    offsets = np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)
    S = int(offsets[-1])
    xyz = np.zeros((S, 3), np.float64)
    face = np.repeat(np.arange(len(f)), n * n).astype(np.int32)
    for nn in np.unique(n[n > 0]).tolist():
        F = np.nonzero(n == nn)[0]
        p, q, w = (a.astype(np.float64)[None, :, None] for a in weights(nn))
        for lo in range(0, len(F), max(1, (1 << 20) // (nn * nn))):
            G = F[lo:lo + max(1, (1 << 20) // (nn * nn))]
            A, B, C = (v[f[G, k]][:, None, :] for k in range(3))
            x = ((p * A + q * B) + w * C) / np.float64(3 * nn)
            xyz[(offsets[G][:, None] + np.arange(nn * nn)[None, :]).ravel()] = x.reshape(-1, 3)
    return (xyz.astype(np.float32) if rounded else xyz), face, offsets


def face_error_numpy(e, face, m):
    """(sum [m] int64, keyed [m] int32, worst [m] int32), one np.add.at / np.maximum.at per output."""
    e, face = np.asarray(e, np.int64), np.asarray(face, np.int64)
    ok = e >= 0
    total, keyed, worst = np.zeros(m, np.int64), np.zeros(m, np.int64), np.full(m, -1, np.int64)
    np.add.at(total, face[ok], e[ok])
    np.add.at(keyed, face[ok], 1)
    np.maximum.at(worst, face[ok], e[ok])
    return total, keyed.astype(np.int32), worst.astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------
# files, restated record by record
# ----------------------------------------------------------------------------------------
def error_mesh_numpy(vertices, faces, total, keyed):
    head = ("ply\nformat binary_little_endian 1.0\ncomment error mesh (deep3d_aerial_amd.mesh_compare)\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nelement face %d\nproperty list uchar int vertex_indices\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (len(vertices), len(faces))).encode("ascii")
    body = b"".join(struct.pack("<3f", *[float(c) for c in p]) for p in np.asarray(vertices, np.float32))
    for tri, t, k in zip(np.asarray(faces).tolist(), [int(x) for x in total], [int(x) for x in keyed]):
        E = t // k if k else None
        rgb = (128, 128, 128) if E is None else (min(255, E >> 1), min(255, (1024 - E) >> 1), 0)
        body += struct.pack("<B3i3B", 3, tri[0], tri[1], tri[2], *rgb)
    return head + body


def samples_numpy(xyz, face):
    head = ("ply\nformat binary_little_endian 1.0\ncomment mesh samples (deep3d_aerial_amd.mesh_compare)\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty int face\nend_header\n" % len(face)).encode("ascii")
    return head + b"".join(struct.pack("<3fi", float(p[0]), float(p[1]), float(p[2]), int(k)) for p, k in zip(np.asarray(xyz, np.float32), face))


# ----------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------
def one_face(n, seed=0):
    """(vertices, faces, spacing): one scalene face in general position whose rule gives n_f = n."""
    rng = np.random.default_rng(seed)
    v = (np.float64([[0.3, -0.2, 1.0], [4.1, 0.4, 1.7], [1.2, 3.3, 0.6]]) + rng.normal(0, 0.01, (3, 3))).astype(np.float32)
    f = np.int32([[0, 1, 2]])
    d = v.astype(np.float64)
    L = max(np.linalg.norm(d[a] - d[b]) for a, b in ((0, 1), (1, 2), (2, 0)))
    s = L / (n - 0.5) if n > 1 else 2.0 * L
    assert counts_numpy(v, f, s)[0].tolist() == [n]
    return v, f, s


def unit_faces(k, seed=0, origin=0.0):
    """(vertices [3k,3], faces [k,3]): k separate small faces, each with n_f = 1 at spacing 1 (longest edge about 0.6)."""
    rng = np.random.default_rng(seed)
    base = np.stack([origin + np.arange(k) % 97 * 1.0, np.arange(k) // 97 * 1.0, rng.uniform(0, 1, k)], 1)
    tri = np.float64([[0, 0, 0], [0.6, 0, 0.05], [0.1, 0.4, 0]])
    v = (base[:, None, :] + tri[None, :, :] + rng.uniform(-0.02, 0.02, (k, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * k, dtype=np.int32).reshape(k, 3)


def big_face(n, at, spacing=1.0):
    """(vertices [3,3], faces [1,3]): one face with n_f = n at `spacing`, placed at x = at."""
    L = (n - 0.5) * spacing
    v = np.float32([[at, -50.0, 0.5], [at + L, -50.0, 1.0], [at + 0.3 * L, -50.0 - 0.6 * L, 0.0]])
    assert counts_numpy(v, np.int32([[0, 1, 2]]), spacing)[0].tolist() == [n]
    return v, np.int32([[0, 1, 2]])


def empty_faces(k, seed=0):
    """(vertices, faces): k faces without samples: zero-length ones (three equal corners, by index and by value) and ones with a
    NaN or an infinite corner, mixed."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 5, (3 * k, 3)).astype(np.float32)
    kind = np.arange(k) % 4
    v[3 * np.arange(k) + 1] = np.where((kind == 0)[:, None], v[3 * np.arange(k)], v[3 * np.arange(k) + 1])
    v[3 * np.arange(k) + 2] = np.where((kind == 0)[:, None], v[3 * np.arange(k)], v[3 * np.arange(k) + 2])
    v[3 * np.arange(k)[kind == 1] + 1, 1] = NAN
    v[3 * np.arange(k)[kind == 2] + 2, 0] = INF
    f = np.arange(3 * k, dtype=np.int32).reshape(k, 3)
    f[kind == 3] = f[kind == 3][:, :1]   # one vertex three times
    assert not counts_numpy(v, f, 1.0)[0].any()
    return v, f


def join(parts):
    """One mesh of the (vertices, faces) parts, in their order."""
    vs, fs, at = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int32).reshape(-1, 3) + at)
        at += len(vs[-1])
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def height_field(seed=0, side=101):
    """(vertices, faces, reference, border, cap, spacing): a gently curved height-field mesh over 40 x 40 of about 2 (side - 1)^2
    faces of mixed sizes (a grid whose lines are unevenly spaced and whose nodes are jittered), and a reference cloud of about 30 000
    points on the same surface, jittered, with 200 floaters and a few points outside the border."""
    rng = np.random.default_rng(seed)
    surf = lambda x, y: 3.0 + 0.8 * np.sin(0.15 * x) * np.cos(0.12 * y)
    lines = lambda: np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 1.7, side - 1))])
    gx, gy = lines(), lines()
    gx, gy = gx * 40.0 / gx[-1], gy * 40.0 / gy[-1] - 20.0
    X, Y = np.meshgrid(gx, gy, indexing="xy")
    X[1:-1, 1:-1] += rng.uniform(-0.05, 0.05, (side - 2, side - 2))
    Y[1:-1, 1:-1] += rng.uniform(-0.05, 0.05, (side - 2, side - 2))
    v = np.stack([X, Y, surf(X, Y)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(side - 1), np.arange(side - 1), indexing="xy")
    a = (j * side + i).ravel()
    flip = rng.random(len(a)) < 0.5
    t1 = np.where(flip[:, None], np.stack([a, a + 1, a + side + 1], 1), np.stack([a, a + 1, a + side], 1))
    t2 = np.where(flip[:, None], np.stack([a, a + side + 1, a + side], 1), np.stack([a + 1, a + side + 1, a + side], 1))
    f = np.concatenate([t1, t2]).astype(np.int32)
    f = f[rng.permutation(len(f))]
    nref = 30000
    x, y = rng.uniform(0, 38, nref), rng.uniform(-20, 20, nref)
    ref = np.concatenate([np.stack([x, y, surf(x, y) + rng.normal(0, 0.04, nref)], 1), rng.uniform([0, -20, 0], [40, 20, 6], (200, 3)),
                          rng.uniform([-5, -25, -3], [45, 25, 9], (20, 3))])
    ref = ref[rng.permutation(len(ref))].astype(np.float32)
    return v, f, ref, [0.0, 40.0, -20.0, 20.0, 0.0, 6.0], 0.5, 0.25


def ply_mesh_bytes(vertices, faces):
    """A mesh as mesh.write_ply writes it."""
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(vertices), len(faces))).encode("ascii")
    return head + np.asarray(vertices, "<f4").tobytes() + b"".join(struct.pack("<B3i", 3, *tri) for tri in np.asarray(faces).tolist())
