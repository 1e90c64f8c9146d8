"""CPU checks of the comparison of a surface mesh with a reference cloud (deep3d_aerial_amd/mesh_compare.py, csrc/mesh_sample.hip,
DESIGN.md §4.30): the numpy restatement of the sampling rule (tests/mesh_compare_scene.py) on its own properties and on hand-computed
cases -- tests/test_mesh_compare_gpu.py compares the kernels against it bit for bit --, the error mesh's bytes, the command line's
refusals, the C ABI and its argument checks, the operators' refusals and the source."""
import ctypes
import itertools
import math
import re
import struct

import numpy as np
import pytest
import torch

import mesh_compare_scene as MS
import test_cloud as TC
from deep3d_aerial_amd import _lib, mesh_compare as MC

NEW_SYMBOLS = ("d3d_mesh_sample_scratch_bytes", "d3d_mesh_sample_count", "d3d_mesh_sample_emit", "d3d_mesh_sample_face_error")
NAN, INF = np.nan, np.inf


# ----------------------------------------------------------------------------------------
# the restatement on its own properties
# ----------------------------------------------------------------------------------------
def random_faces(seed, k, slivers=True):
    """k separate faces of mixed sizes; with slivers every fourth face is one (a height of a hundredth of its base, or less)."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-5, 5, (k, 3))
    u = rng.normal(size=(k, 3)) * rng.uniform(0.2, 4.0, (k, 1))
    w = rng.normal(size=(k, 3)) * rng.uniform(0.2, 4.0, (k, 1))
    if slivers:
        thin = np.arange(k) % 4 == 0
        w = np.where(thin[:, None], u * rng.uniform(0.1, 0.9, (k, 1)) + w * 1e-3, w)
    v = np.stack([A, A + u, A + w], 1).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * k, dtype=np.int32).reshape(k, 3)


@pytest.mark.parametrize("n", list(range(1, 41)))
def test_the_weights_are_distinct_positive_and_sum_to_3n(n):
    p, q, w = MS.weights(n)
    assert len(p) == n * n and (p > 0).all() and (q > 0).all() and (w > 0).all() and ((p + q + w) == 3 * n).all()
    assert len({(int(a), int(b)) for a, b in zip(p, q)}) == n * n
    # n (n + 1) / 2 upright and n (n - 1) / 2 inverted sub-triangles: their centroids have weights = 1 and = 2 (mod 3)
    assert (p % 3 == 1).sum() == n * (n + 1) // 2 and (p % 3 == 2).sum() == n * (n - 1) // 2
    assert ((p % 3 == q % 3) & (q % 3 == w % 3)).all()


def test_the_integer_square_root_is_exact_around_every_square():
    r = np.arange(1, 32769, dtype=np.int64)
    for d in (-1, 0, 1):
        assert np.array_equal(MS.isqrt_numpy(r * r + d), r - (d < 0))
    assert MS.isqrt_numpy([0, 1, 2, 3, 4, (1 << 30) - 1, 1 << 30]).tolist() == [0, 1, 1, 1, 2, 32767, 32768]


def test_n_squared_samples_per_face_inside_it_and_in_face_order():
    v, f = random_faces(1, 300, slivers=False)
    s = 0.7
    n, clipped = MS.counts_numpy(v, f, s)
    xyz, face, offsets = MS.sample_numpy(v, f, s, rounded=False)
    assert not clipped.any() and n.min() >= 1 and n.max() > 5 and len(np.unique(n)) > 5
    assert np.array_equal(np.diff(offsets), n * n) and offsets[0] == 0 and len(xyz) == offsets[-1] == len(face)
    assert np.array_equal(face, np.repeat(np.arange(len(f)), n * n)) and face.dtype == np.int32
    # inside: the three sub-triangles a sample makes with the face's edges have the face's area together
    d = v.astype(np.float64)
    A, B, C = (d[f[face, k]] for k in range(3))
    area = lambda a, b, c: 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    parts = area(xyz, A, B) + area(xyz, B, C) + area(xyz, C, A)
    assert (parts <= area(A, B, C) * (1 + 1e-9)).all()
    r32 = MS.sample_numpy(v, f, s)[0]
    assert r32.dtype == np.float32 and np.array_equal(r32, xyz.astype(np.float32))


def test_every_point_of_a_face_is_within_two_thirds_of_the_spacing_of_a_sample_of_it():
    rng = np.random.default_rng(2)
    v, f = random_faces(3, 400)
    worst = 0.0
    for s in (0.35, 1.0, 3.0):
        xyz, face, offsets = MS.sample_numpy(v, f, s, rounded=False)
        d = v.astype(np.float64)
        for k in range(len(f)):
            b = rng.dirichlet([0.6, 0.6, 0.6], 40)   # corners and edges too
            b[:3] = np.eye(3)
            pts = b @ d[f[k]]
            own = xyz[offsets[k]:offsets[k + 1]]
            near = np.sqrt(((pts[:, None, :] - own[None, :, :]) ** 2).sum(-1).min(1)).max()
            worst = max(worst, near / s)
            assert near <= 2.0 * s / 3.0 * (1 + 1e-9), (k, s, near)
    # the bound is not idle: the far corner of a sliver whose longest edge is nearly n s is nearly 2/3 of it from the centroid
    assert worst > 0.5


def test_the_sample_multiset_does_not_depend_on_the_face_order():
    v, f = random_faces(4, 500)
    s = 0.8
    xyz, face, _ = MS.sample_numpy(v, f, s)
    perm = np.random.default_rng(5).permutation(len(f))
    xyz2, face2, _ = MS.sample_numpy(v, f[perm], s)
    key = lambda a: np.sort(np.ascontiguousarray(MS.bits(a)).view([("x", "<u4"), ("y", "<u4"), ("z", "<u4")]).ravel())
    assert np.array_equal(key(xyz), key(xyz2)) and not np.array_equal(xyz, xyz2)
    # and a face's samples are the same wherever it stands
    inv = np.argsort(perm)
    by_face = lambda x, fc, k: x[fc == k]
    for k in (0, 17, 499):
        assert np.array_equal(by_face(xyz, face, k), by_face(xyz2, face2, inv[k]))


# ----------------------------------------------------------------------------------------
# hand cases (shared with tests/test_mesh_compare_gpu.py)
# ----------------------------------------------------------------------------------------
def hand_cases():
    """(name, vertices, faces, spacing, n per face, samples or None) worked out by hand."""
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0]])   # edges 1, sqrt(0.5), sqrt(0.5)
    f = np.int32([[0, 1, 2]])
    third = np.float64(1.0) / 3.0
    return [
        # n = 1: ((1 A + 1 B) + 1 C) / 3
        ("n = 1: the centroid", np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), f, 2.0, [1], [[np.float32(third), np.float32(third), 0.0]]),
        # edges 6, sqrt(45) = 6.7.., 3; s = 4: q = 1.67.., n = 2, 3n = 6:
        #   t = 0: r = 0, c = 0: (4, 1, 1);  t = 1: r = 1, c = 0, k = 0: (1, 1, 4);  t = 2: c = 1: (2, 2, 2);  t = 3: c = 2, k = 1: (1, 4, 1)
        ("n = 2: four points", np.float32([[0, 0, 0], [6, 0, 0], [0, 3, 0]]), f, 4.0, [2], [[1, 0.5, 0], [1, 2, 0], [2, 1, 0], [4, 0.5, 0]]),
        ("an edge of exactly s", tri, f, 1.0, [1], [[0.5, np.float32(np.float64(0.5) / 3.0), 0]]),
        # s = 1 / (1 + 2^-40): q = 1 / s = 1 + 2^-40 > 1, n = ceil(q) = 2
        ("an edge of s (1 + 2^-40)", tri, f, 1.0 / (1.0 + 2.0 ** -40), [2], None),
        ("a zero-length face", np.float32([[1, 2, 3], [1, 2, 3], [1, 2, 3]]), f, 1.0, [0], []),
        ("one vertex three times", tri, np.int32([[1, 1, 1]]), 1.0, [0], []),
        # (0,0,0) (1,0,0) (2,0,0): L = 2, n = 2; (4A + B + C) / 6 = 0.5, (A + B + 4C) / 6 = 1.5, (2A + 2B + 2C) / 6 = 1, (A + 4B + C) / 6 = 1
        ("a collinear face with L > 0 is sampled", np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), f, 1.0, [2],
         [[0.5, 0, 0], [1.5, 0, 0], [1, 0, 0], [1, 0, 0]]),
        ("a NaN corner", np.float32([[0, 0, 0], [1, NAN, 0], [0, 1, 0]]), f, 1.0, [0], []),
        ("an infinite corner", np.float32([[0, 0, 0], [1, 0, 0], [0, -INF, 0]]), f, 1.0, [0], []),
        ("a NaN corner beside a sampled face", np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [NAN, 0, 0]]), np.int32([[0, 1, 3], [0, 1, 2], [3, 3, 3]]),
         2.0, [0, 1, 0], [[np.float32(third), np.float32(third), 0.0]]),
    ]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_the_rule_by_hand(case):
    _, v, f, s, n, want = case
    got_n, clipped = MS.counts_numpy(v, f, s)
    assert got_n.tolist() == n and not clipped.any()
    xyz, face, offsets = MS.sample_numpy(v, f, s)
    assert offsets.tolist() == [0] + np.cumsum(np.square(n)).tolist() and xyz.shape == (offsets[-1], 3)
    if want is not None:
        assert np.array_equal(MS.bits(xyz), MS.bits(np.float32(want).reshape(-1, 3)))
    assert face.tolist() == [k for k, nn in enumerate(n) for _ in range(nn * nn)]


def test_a_face_longer_than_32768_spacings_is_clipped():
    v = np.float32([[0, 0, 0], [32768, 0, 0], [0, 1, 0]])
    f = np.int32([[0, 1, 2]])
    n, clipped = MS.counts_numpy(v, f, 1.0)     # L = sqrt(32768^2 + 1) > 32768
    assert n.tolist() == [32768] and clipped.tolist() == [True]
    n, clipped = MS.counts_numpy(np.float32([[0, 0, 0], [32768, 0, 0], [0, 0, 0]]), f, 1.0)   # L = 32768 exactly: the largest n_f
    assert n.tolist() == [32768] and clipped.tolist() == [False]
    n, clipped = MS.counts_numpy(v, f, 1e-300)   # q overflows
    assert n.tolist() == [32768] and clipped.tolist() == [True]


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def test_the_error_mesh_bytes_by_hand():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    f = np.int32([[0, 1, 2], [1, 3, 2], [0, 0, 0], [2, 1, 0]])
    total = np.int64([0, 3 * 1024, 0, 1023])
    keyed = np.int32([5, 3, 0, 2])
    data = MC.error_mesh_bytes(v, f, total, keyed)
    assert data == MS.error_mesh_numpy(v, f, total, keyed)
    assert data == MC.error_mesh_bytes(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(total), torch.from_numpy(keyed))
    end = data.index(b"end_header\n") + 11
    assert data[:end].decode().split("\n")[3:12] == ["element vertex 4", "property float x", "property float y", "property float z", "element face 4",
                                                     "property list uchar int vertex_indices", "property uchar red", "property uchar green",
                                                     "property uchar blue"]
    body = data[end:]
    assert len(body) == 4 * 12 + 4 * 16 and body[:48] == v.tobytes()
    rows = [struct.unpack_from("<B3i3B", body, 48 + 16 * k) for k in range(4)]
    assert rows[0] == (3, 0, 1, 2, 0, 255, 0)          # E = 0: on the reference
    assert rows[1] == (3, 1, 3, 2, 255, 0, 0)          # E = 1024: at the cap
    assert rows[2] == (3, 0, 0, 0, 128, 128, 128)      # no keyed sample: grey
    assert rows[3] == (3, 2, 1, 0, 255, 255, 0)        # E = 1023 // 2 = 511: 511 >> 1 = 255, 513 >> 1 = 256 -> 255
    assert MC.error_mesh_bytes(v, f[:0], total[:0], keyed[:0]).endswith(v.tobytes())
    for bad in ((v.astype(np.float64), f, total, keyed), (v, f.astype(np.int64), total, keyed), (v, f, total.astype(np.int32), keyed),
                (v, f, total, keyed[:3]), (v, f, total, np.int32([5, 2, 0, 2])), (v, f, -total, keyed), (v, f, total, -keyed)):
        with pytest.raises(ValueError):
            MC.error_mesh_bytes(*bad)
    xyz, face = np.float32([[1, 2, 3], [4, 5, 6]]), np.int32([7, 9])
    assert MC.samples_bytes(xyz, face) == MS.samples_numpy(xyz, face) and MC.samples_bytes(xyz, face).endswith(struct.pack("<3fi", 4, 5, 6, 9))
    with pytest.raises(ValueError):
        MC.samples_bytes(xyz, face.astype(np.int64))


def test_the_command_line_refuses_before_it_reads_or_writes(capsys, tmp_path):
    a, b = str(tmp_path / "m.ply"), str(tmp_path / "b.ply")   # neither exists: a refusal comes before any read
    out = tmp_path / "out"
    full = ["--mesh", a, "--reference", b, "--border=0,8,0,4,-1,1", "--max_dist=0.5", "--threshold=0.1,0.25", "--spacing=0.05",
            "--json", str(out / "r.json"), "--out_samples", str(out / "s.ply"), "--out_accuracy", str(out / "ea.ply"),
            "--out_completeness", str(out / "eb.ply"), "--out_mesh", str(out / "em.ply")]
    sub = lambda k, *new: full[:k] + list(new) + full[k + (1 if full[k].count("=") else 2):]
    for argv in (sub(0), sub(2), sub(4), sub(5), sub(6), sub(7),
                 sub(4, "--border=0,8,0,4"), sub(5, "--max_dist=0"), sub(6, "--threshold=0.1,0.5"), sub(6, "--threshold=0.1,x"),
                 sub(7, "--spacing=0"), sub(7, "--spacing=-1"), sub(7, "--spacing=nan"), sub(7, "--spacing=inf"),
                 sub(8, "--json", str(out / "r.txt")), sub(10, "--out_samples", str(out / "s.xyz")), sub(12, "--out_accuracy", str(out / "ea.obj")),
                 sub(14, "--out_completeness", str(out / "eb")), sub(16, "--out_mesh", str(out / "em.json")),
                 sub(16, "--out_mesh", str(out / "s.ply")), sub(12, "--out_accuracy", str(out / "eb.ply")),
                 sub(16, "--out_mesh", a), sub(10, "--out_samples", b),
                 full + ["--cloud", a]):
        with pytest.raises(SystemExit):
            MC.main(argv)
    err = capsys.readouterr().err
    for text in ("--mesh is required", "--reference is required", "--border is required", "--max_dist is required", "--threshold is required",
                 "--spacing is required", "max_dist must be finite", "1 .. 1023", "T[,T...]", "spacing must be finite", "--json must end in .json",
                 "--out_samples must end in .ply", "--out_accuracy must end in .ply", "--out_completeness must end in .ply",
                 "--out_mesh must end in .ply", "the same file", "overwrite an input", "unrecognized arguments"):
        assert text in err, text
    assert err.count("the same file") == 2 and err.count("overwrite an input") == 2 and err.count("spacing must be finite") == 4
    assert not out.exists() and list(tmp_path.iterdir()) == []


# ----------------------------------------------------------------------------------------
# the library and the operators
# ----------------------------------------------------------------------------------------
def test_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    assert sorted(_lib.STRUCTS) == ["d3d_mesh_grid_t", "d3d_mesh_view_t", "d3d_ortho_view_t"]   # no new struct
    assert [len(_lib.SIGNATURES[s]) for s in NEW_SYMBOLS[1:]] == [11, 9, 8]
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_build_flags() == b""
    scratch = lib.d3d_mesh_sample_scratch_bytes
    assert scratch.restype is ctypes.c_size_t
    big = (1 << 31) - 1
    tiles = lambda m: (m + 4095) // 4096
    assert scratch(0) > 0 and scratch(1) >= 8 and scratch(1_000_000) >= 8 * tiles(1_000_000) and scratch(big) >= 8 * tiles(big)
    for bad in (-1, 1 << 31, -(1 << 40), 1 << 40):
        assert scratch(bad) == 0, bad


def _alias(ok, size):
    """Every pair of buffers, both ways: one begins on the last byte of the other."""
    cases = []
    for a, b in itertools.combinations(size, 2):
        cases.append((dict([(b, ctypes.c_void_p(ok[a].value + size[a] - 1))]), b"alias"))
        cases.append((dict([(a, ctypes.c_void_p(ok[b].value + size[b] - 1))]), b"alias"))
    return cases


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    nv, m, S = 9, 7, 10
    bad_n = lambda name, msg: [(dict([(name, -1)]), msg), (dict([(name, 1 << 31)]), msg)]
    # count
    need = lib.d3d_mesh_sample_scratch_bytes(m)
    order = ["v", "nv", "f", "m", "sp", "s", "sb", "counts", "offsets", "totals", "st"]
    ok = dict(v=P(1), nv=nv, f=P(2), m=m, sp=0.25, s=P(3), sb=need, counts=P(4), offsets=P(5), totals=P(6), st=None)
    size = dict(v=12 * nv, f=12 * m, s=need, counts=4 * m, offsets=4 * (m + 1), totals=16)
    alias = _alias(ok, size)
    assert len(alias) == 30
    TC._expect(lib, lib.d3d_mesh_sample_count, ok, order,
               [(dict([(name, None)]), b"null") for name in size] + bad_n("nv", b"n_vertices") + bad_n("m", b"n_faces") +
               [(dict(sp=0.0), b"spacing"), (dict(sp=-1.0), b"spacing"), (dict(sp=math.nan), b"spacing"), (dict(sp=math.inf), b"spacing"),
                (dict(sp=-math.inf), b"spacing"), (dict(sb=need - 1), b"scratch"), (dict(sb=0), b"scratch"),
                # no face: the scratch, the offsets and the totals are still needed
                (dict(m=0, f=None, counts=None, s=None), b"null"), (dict(m=0, f=None, counts=None, offsets=None), b"null"),
                (dict(m=0, f=None, counts=None, totals=None), b"null"), (dict(m=0, sb=0), b"scratch")] + alias)
    # emit
    order = ["v", "nv", "f", "m", "offsets", "S", "xyz", "face", "st"]
    ok = dict(v=P(1), nv=nv, f=P(2), m=m, offsets=P(3), S=S, xyz=P(4), face=P(5), st=None)
    size = dict(v=12 * nv, f=12 * m, offsets=4 * (m + 1), xyz=12 * S, face=4 * S)
    alias = _alias(ok, size)
    assert len(alias) == 20
    TC._expect(lib, lib.d3d_mesh_sample_emit, ok, order,
               [(dict([(name, None)]), b"null") for name in size] + bad_n("nv", b"n_vertices") + bad_n("m", b"n_faces") + bad_n("S", b"n_samples") +
               [(dict(m=0, f=None), b"n_samples"), (dict(m=0, S=0, f=None, xyz=None, face=None, offsets=None), b"null")] + alias)
    # face error
    order = ["e", "face", "S", "m", "sum", "keyed", "worst", "st"]
    ok = dict(e=P(1), face=P(2), S=S, m=m, sum=P(3), keyed=P(4), worst=P(5), st=None)
    size = dict(e=4 * S, face=4 * S, sum=8 * m, keyed=4 * m, worst=4 * m)
    alias = _alias(ok, size)
    assert len(alias) == 20
    TC._expect(lib, lib.d3d_mesh_sample_face_error, ok, order,
               [(dict([(name, None)]), b"null") for name in size] + bad_n("S", b"n_samples") + bad_n("m", b"n_faces") +
               [(dict(S=0, e=None, face=None, sum=None), b"null"), (dict(m=0, sum=None, keyed=None, worst=None, e=None), b"null")] + alias)
    # what is valid without a launch: no face and no sample
    assert lib.d3d_mesh_sample_emit(None, 0, None, 0, P(3), 0, None, None, None) == 0
    assert lib.d3d_mesh_sample_face_error(None, None, 0, 0, None, None, None, None) == 0
    assert lib.d3d_mesh_sample_face_error(P(1), P(2), S, 0, None, None, None, None) == 0


def test_the_operators_refuse_cpu_tensors_bad_dtypes_and_shapes():
    v, f = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    ref = torch.zeros(5, 3)
    border = [0.0, 4.0, 0.0, 4.0, 0.0, 4.0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.sample(v, f, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.face_error(torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.compare(v, f, ref, border, 1.0, [0.5], 0.5)
    for s in (0.0, -1.0, NAN, INF, "1", True, None):
        with pytest.raises(ValueError, match="spacing"):
            MC.sample(v, f, s)
        with pytest.raises(ValueError, match="spacing"):
            MC.compare(v, f, ref, border, 1.0, [0.5], s)
    for k in (-1, 1 << 31, 2.5, True, None):
        with pytest.raises(ValueError, match="max_samples"):
            MC.sample(v, f, 0.5, max_samples=k)
    with pytest.raises(TypeError, match="tensors"):
        MC.sample(np.zeros((4, 3), np.float32), f, 0.5)
    with pytest.raises(TypeError, match="tensors"):
        MC.face_error(np.zeros(6, np.int32), torch.zeros(6, dtype=torch.int32), 2)
    e = torch.zeros(6, dtype=torch.int32)
    for bad_e, bad_face in ((e.long(), e), (e, e.long()), (e, e[:5]), (e.reshape(2, 3), e.reshape(2, 3)), (e.float(), e)):
        with pytest.raises(ValueError, match="int32"):
            MC.face_error(bad_e, bad_face, 2)
    for k in (-1, 1 << 31, 2.0, True):
        with pytest.raises(ValueError, match="n_faces"):
            MC.face_error(e, e, k)
    for bad in (ref.double(), torch.zeros(5, 2), torch.zeros(15), torch.zeros(5, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="reference_xyz"):
            MC.compare(v, f, bad, border, 1.0, [0.5], 0.5)
    with pytest.raises(TypeError, match="Tensor"):
        MC.compare(v, f, None, border, 1.0, [0.5], 0.5)
    for kw, msg in ((dict(max_dist=0.0), "max_dist"), (dict(max_dist=1e-9, thresholds=[5e-10]), "2\\^21"), (dict(border=[0, 4, 0, 4]), "six"),
                    (dict(thresholds=[1.0]), "1 .. 1023"), (dict(thresholds=[]), "at least one")):
        with pytest.raises(ValueError, match=msg):
            MC.compare(**dict(dict(vertices=v, faces=f, reference_xyz=ref, border=border, max_dist=1.0, thresholds=[0.5], spacing=0.5), **kw))


def test_the_kernels_use_integer_atomics_only_no_fma_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/mesh_sample.hip").read())
    assert set(re.findall(r"\batomic\w*", hip)) == {"atomicAdd", "atomicMax"}
    assert not re.search(r"unsafeAtomic|atomic(Add|Max)\s*\(\s*\(?\s*(float|double)\s*\*|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
    # every atomic is a statement (its result is not used) on an integer array: the two totals, and sum, keyed and worst
    calls = re.findall(r"\batomic(?:Add|Max)\(([^,]+),", hip)
    assert len(re.findall(r"(?:^|[;{}\)])\s*atomic(?:Add|Max)\(", hip, re.M)) == len(calls) == 5
    assert sorted(c.strip() for c in calls) == ["keyed + f", "sum + f", "totals", "totals + 1", "worst + f"]
    assert re.search(r"unsigned long long\* __restrict__ totals\)", hip) and re.search(r"unsigned long long\* __restrict__ sum,", hip)
    assert re.search(r"int\* __restrict__ keyed, int\* __restrict__ worst\)", hip)
    assert "fma" not in hip and "asm" not in hip and "printf" not in hip and "assert" not in hip
    # the pieces it reuses are included, not restated
    assert '#include "cloud_search.h"' in hip and '#include "geom_shared.h"' in hip and "search_apart(" in hip and "geom_scan(" in hip
    assert "geom_face<false>(" in hip and "geom_load3(" in hip and "struct SearchRange" not in hip
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bmesh_sample\.hip\b", make, re.M) and "-ffp-contract=off" in make
    assert "D3D_MESH_SAMPLE_PLAIN" in make   # the variant the bench times beside the production form
