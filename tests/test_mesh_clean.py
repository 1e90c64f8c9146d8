"""Mesh cleaning without a GPU: a numpy restatement of the rules of deep3d_aerial_amd/mesh.py (edges and
adjacency, components, removal, smoothing), checked on hand cases; the new flags of predict and of the mesh command line; the
new entry points refusing null pointers and bad sizes before any launch.  tests/test_mesh_clean_gpu.py holds the kernels to
this restatement bit for bit."""
import ctypes

import numpy as np
import pytest

from deep3d_aerial_amd import _lib, mesh


# ----------------------------------------------------------------------------------------
# the numpy restatement
# ----------------------------------------------------------------------------------------
def edges_numpy(faces):
    """(lo, hi, multiplicity) of every distinct edge: the unordered pairs of (a,b) (b,c) (c,a) with unequal ends, once per face."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = f.shape[0]
    p = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1)
    lo, hi = p.min(2).ravel(), p.max(2).ravel()
    fid = np.repeat(np.arange(m), 3)
    ok = lo != hi
    per_face = np.unique(np.stack([fid[ok], lo[ok], hi[ok]], 1), axis=0) if ok.any() else np.zeros((0, 3), np.int64)
    e, cnt = np.unique(per_face[:, 1:], axis=0, return_counts=True) if len(per_face) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    return e[:, 0], e[:, 1], cnt


def adjacency_numpy(n, faces):
    """(offset [n+1] int64, nbr int32, fixed [n] uint8)."""
    lo, hi, cnt = edges_numpy(faces)
    src, dst, mult = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([cnt, cnt])
    order = np.lexsort((dst, src))
    src, dst, mult = src[order], dst[order], mult[order]
    deg = np.bincount(src, minlength=n)
    offset = np.zeros(n + 1, np.int64)
    offset[1:] = np.cumsum(deg)
    fixed = deg == 0
    fixed[src[mult != 2]] = True
    return offset, dst.astype(np.int32), fixed.astype(np.uint8)


def components_numpy(n, faces):
    """label [n] int32: the smallest vertex index of each vertex's component (faces connect through shared vertices)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    r = np.concatenate([f[:, 0], f[:, 0]])
    c = np.concatenate([f[:, 1], f[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(r)), (r, c)), shape=(n, n)), directed=False)
    mins = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(mins, comp, np.arange(n))
    return mins[comp].astype(np.int32)


def _diag(box):
    b = box.astype(np.float64)
    dx, dy, dz = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def stats_numpy(vertices, faces, label):
    """face_count [n], box [n,6] fp32 (NaN where no vertex has the label), diag [n] fp64, global box [6], global diag."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = v.shape[0]
    count = np.bincount(label[f[:, 0]], minlength=n).astype(np.int32) if len(f) else np.zeros(n, np.int32)
    lo = np.full((n, 3), np.inf, np.float32)
    hi = np.full((n, 3), -np.inf, np.float32)
    np.minimum.at(lo, label, v)
    np.maximum.at(hi, label, v)
    box = np.concatenate([lo, hi], 1)
    box[~np.isfinite(box[:, 0])] = np.nan
    used = np.unique(f)
    gbox = (np.concatenate([v[used].min(0), v[used].max(0)]) if len(used) else np.full(6, np.nan)).astype(np.float32)
    return count, box, _diag(box), gbox, float(_diag(gbox))


def remove_numpy(vertices, faces, min_faces=0, spurious=0.0):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    n = v.shape[0]
    label = components_numpy(n, f)
    count, _, diag, _, gdiag = stats_numpy(v, f, label)
    r = label[f[:, 0]]
    gone = np.zeros(len(f), bool)
    if min_faces > 0:
        gone |= count[r] < min_faces
    if spurious > 0:
        gone |= diag[r] < gdiag / spurious
    kf = f[~gone]
    keep = np.zeros(n, bool)
    keep[kf.ravel()] = True
    remap = np.cumsum(keep) - 1
    return v[keep], remap[kf].astype(np.int32).reshape(-1, 3)


def smooth_numpy(vertices, faces, iterations, lam=0.5):
    """Jacobi iterations: sums over the padded neighbour matrix column by column in fp32 (the kernel's increasing order)."""
    x = np.asarray(vertices, np.float32).reshape(-1, 3).copy()
    n = x.shape[0]
    offset, nbr, fixed = adjacency_numpy(n, faces)
    deg = np.diff(offset)
    width = int(deg.max()) if n else 0
    cols = np.zeros((n, width), np.int64)
    valid = np.arange(width)[None, :] < deg[:, None]
    cols[valid] = nbr
    lam = np.float32(lam)
    move = fixed == 0
    c = deg.astype(np.float32)[:, None]
    for _ in range(iterations):
        s = np.zeros_like(x)
        for k in range(width):
            s = np.where(valid[:, k:k + 1], s + x[cols[:, k]], s)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = s / c
        x = np.where(move[:, None], x + lam * (mean - x), x).astype(np.float32)
    return x


def clean_numpy(vertices, faces, min_faces=0, spurious=0.0, smooth=0, lam=0.5):
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    if min_faces > 0 or spurious > 0:
        v, f = remove_numpy(v, f, min_faces, spurious)
    if smooth > 0:
        v = smooth_numpy(v, f, smooth, lam)
    return v, f


# ----------------------------------------------------------------------------------------
# hand cases (shared with the GPU tests)
# ----------------------------------------------------------------------------------------
def _tetra():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
    return v, f


def _fan(k=6):
    ang = np.arange(k) * 2 * np.pi / k
    v = np.concatenate([[[0, 0, 0.5]], np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], 1)]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)
    return v, f


def _two_pieces():
    """A big fan (12 faces, radius 10) and a small tetrahedron (4 faces, size 1) floating away from it."""
    vb, fb = _fan(12)
    vb = vb * np.float32(10)
    vt, ft = _tetra()
    vt = vt + np.float32([3, 3, 5])
    return np.concatenate([vt, vb]), np.concatenate([ft, fb + 4]).astype(np.int32)


HAND = {
    "two_triangles": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32), np.array([[0, 1, 2], [1, 3, 2]], np.int32)),
    "tetrahedron": _tetra(),
    "fan": _fan(),
    "two_pieces": _two_pieces(),
    "repeated_index": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2]], np.float32), np.array([[0, 1, 2], [1, 1, 3]], np.int32)),
    "unreferenced": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [7, 7, 7], [1, 1, 0]], np.float32), np.array([[0, 1, 2], [1, 4, 2]], np.int32)),
}


def test_two_triangles_only_the_shared_edge_is_manifold():
    v, f = HAND["two_triangles"]
    lo, hi, cnt = edges_numpy(f)
    assert dict(zip(zip(lo.tolist(), hi.tolist()), cnt.tolist())) == {(0, 1): 1, (0, 2): 1, (1, 2): 2, (1, 3): 1, (2, 3): 1}
    offset, nbr, fixed = adjacency_numpy(4, f)
    assert offset.tolist() == [0, 2, 5, 8, 10] and nbr.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    assert fixed.tolist() == [1, 1, 1, 1]   # every vertex has a boundary edge
    assert np.array_equal(smooth_numpy(v, f, 3), v)


def test_closed_tetrahedron_has_no_fixed_vertex():
    v, f = HAND["tetrahedron"]
    offset, nbr, fixed = adjacency_numpy(4, f)
    assert offset.tolist() == [0, 3, 6, 9, 12] and nbr.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert fixed.tolist() == [0, 0, 0, 0]
    s = smooth_numpy(v, f, 1)
    # vertex 0: mean of the other three (1/3, 1/3, 1/3), half way
    assert np.array_equal(s[0], np.float32(0.5) * (np.float32([1, 1, 1]) / np.float32(3)))
    assert np.array_equal(s[1], np.float32([1, 0, 0]) + np.float32(0.5) * (np.float32([0, 1, 1]) / np.float32(3) - np.float32([1, 0, 0])))


def test_fan_centre_is_free_and_the_rim_is_fixed():
    v, f = HAND["fan"]
    offset, nbr, fixed = adjacency_numpy(7, f)
    assert nbr[offset[0]:offset[1]].tolist() == [1, 2, 3, 4, 5, 6]
    assert fixed.tolist() == [0, 1, 1, 1, 1, 1, 1]
    s = smooth_numpy(v, f, 2)
    assert np.array_equal(s[1:], v[1:])
    assert s[0, 2] == np.float32(0.125) and abs(float(s[0, 0])) < 1e-6   # the centre drops toward the rim's plane: 0.5, 0.25, 0.125


def test_two_pieces_min_faces_and_spurious_each_remove_the_small_one():
    v, f = HAND["two_pieces"]
    label = components_numpy(len(v), f)
    assert label.tolist() == [0] * 4 + [4] * 13
    count, box, diag, gbox, gdiag = stats_numpy(v, f, label)
    assert count[0] == 4 and count[4] == 12 and np.array_equal(box[0], np.float32([3, 3, 5, 4, 4, 6]))
    assert diag[0] == np.sqrt(3.0) and np.isnan(diag[1])
    assert np.array_equal(gbox, np.concatenate([v.min(0), v.max(0)]))
    for kw in ({"min_faces": 5}, {"spurious": 5.0}):
        V, F = remove_numpy(v, f, **kw)
        assert len(V) == 13 and len(F) == 12 and np.array_equal(V, v[4:]) and np.array_equal(F, f[4:] - 4)
    V, F = remove_numpy(v, f, min_faces=4, spurious=20.0)   # thresholds the small piece meets: nothing goes
    assert np.array_equal(V, v) and np.array_equal(F, f)
    V, F = remove_numpy(v, f, min_faces=13)   # every component is smaller: nothing is left
    assert V.shape == (0, 3) and F.shape == (0, 3)
    assert gdiag / 5.0 > np.sqrt(3.0) > gdiag / 20.0


def test_face_with_a_repeated_index_has_one_edge():
    v, f = HAND["repeated_index"]
    lo, hi, cnt = edges_numpy(f)
    assert list(zip(lo.tolist(), hi.tolist(), cnt.tolist())) == [(0, 1, 1), (0, 2, 1), (1, 2, 1), (1, 3, 1)]
    offset, nbr, fixed = adjacency_numpy(4, f)
    assert nbr[offset[1]:offset[2]].tolist() == [0, 2, 3] and nbr[offset[3]:offset[4]].tolist() == [1]
    assert components_numpy(4, f).tolist() == [0, 0, 0, 0]


def test_unreferenced_vertex_is_fixed_its_own_component_and_dropped_by_removal():
    v, f = HAND["unreferenced"]
    offset, nbr, fixed = adjacency_numpy(5, f)
    assert offset[3] == offset[4] and fixed[3] == 1
    label = components_numpy(5, f)
    assert label.tolist() == [0, 0, 0, 3, 0]
    count, box, diag, gbox, gdiag = stats_numpy(v, f, label)
    assert count[3] == 0 and diag[3] == 0.0 and np.array_equal(gbox, np.float32([0, 0, 0, 1, 1, 0]))   # 3 is not in the global box
    V, F = remove_numpy(v, f, min_faces=1)
    assert np.array_equal(V, v[[0, 1, 2, 4]]) and F.tolist() == [[0, 1, 2], [1, 3, 2]]
    assert np.array_equal(smooth_numpy(v, f, 1)[3], v[3])


def test_shuffled_faces_give_the_same_restatement():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((60, 3)).astype(np.float32)
    f = rng.integers(0, 60, (150, 3)).astype(np.int32)
    p = rng.permutation(len(f))
    for a, b in zip(adjacency_numpy(60, f), adjacency_numpy(60, f[p])):
        assert np.array_equal(a, b)
    assert np.array_equal(smooth_numpy(v, f, 3).view(np.int32), smooth_numpy(v, f[p], 3).view(np.int32))
    V1, F1 = remove_numpy(v, f, min_faces=3)
    V2, F2 = remove_numpy(v, f[p], min_faces=3)
    assert np.array_equal(V1, V2) and sorted(map(tuple, F1.tolist())) == sorted(map(tuple, F2.tolist()))


# ----------------------------------------------------------------------------------------
# settings and command lines
# ----------------------------------------------------------------------------------------
def test_clean_settings():
    assert mesh.check_clean_settings() == (0, 0.0, 0, 0.5)
    assert mesh.check_clean_settings(10, 20, 2, 1.0) == (10, 20.0, 2, 1.0)
    for kw, what in (({"min_faces": -1}, "min_faces"), ({"min_faces": 1.5}, "min_faces"), ({"spurious": -1}, "spurious"),
                     ({"spurious": float("inf")}, "spurious"), ({"smooth": -2}, "smooth"), ({"smooth_lambda": 0}, "smooth_lambda"),
                     ({"smooth_lambda": 1.5}, "smooth_lambda"), ({"smooth_lambda": float("nan")}, "smooth_lambda")):
        with pytest.raises(ValueError, match=what):
            mesh.check_clean_settings(**kw)
    # settings dicts without the keys (older callers) mean "off"
    assert not mesh.clean_requested({"path": "x", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1})
    assert mesh.clean_requested({"smooth": 1}) and mesh.clean_requested({"min_faces": 3}) and mesh.clean_requested({"spurious": 2.0})


def test_predict_and_mesh_command_line_flags(capsys):
    from deep3d_aerial_amd import predict

    base = ["--model", "casmvsnet", "--loadckpt", "x.ckpt", "--data_folder", "d", "--output_folder", "o", "--fuse", "--mesh", "m.ply",
            "--mesh_border", "0,1,0,1,0,1", "--mesh_voxel", "0.1"]
    a = predict.parse_args(base)
    s = predict._mesh_settings(a)
    assert (s["min_faces"], s["spurious"], s["smooth"], s["smooth_lambda"]) == (0, 0.0, 0, 0.5) and not mesh.clean_requested(s)
    a = predict.parse_args(base + ["--mesh_min_faces", "20", "--mesh_spurious", "20", "--mesh_smooth", "1", "--mesh_smooth_lambda", "0.3"])
    s = predict._mesh_settings(a)
    assert (s["min_faces"], s["spurious"], s["smooth"], s["smooth_lambda"]) == (20, 20.0, 1, 0.3)
    for bad, what in ((["--mesh_min_faces", "-1"], "min_faces"), (["--mesh_spurious", "-3"], "spurious"), (["--mesh_smooth", "-1"], "smooth"),
                      (["--mesh_smooth_lambda", "2"], "smooth_lambda")):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
        assert what in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--out", "o.ply", "--smooth_lambda", "0"])
    assert "smooth_lambda" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--mvs", "x", "--out", "o.ply"])   # one source only
    capsys.readouterr()
    with pytest.raises(SystemExit):
        mesh.main(["--out", "o.ply", "--min_faces", "3"])   # a source is required
    capsys.readouterr()
    with pytest.raises(SystemExit):
        mesh.main(["--mvs", "x", "--out", "o.ply", "--border", "0,1,0,1,0,1", "--voxel", "0.1", "--spurious", "-1"])
    assert "spurious" in capsys.readouterr().err


def test_new_entry_points_refuse_null_pointers_and_bad_sizes_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(8)
    rounds = ctypes.c_int(0)
    assert lib.d3d_mesh_adjacency(None, 0, 0, None, 0, None, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_mesh_adjacency(p, -1, 4, p, 1 << 20, p, p, p, None) == -1
    assert lib.d3d_mesh_adjacency(p, 1 << 29, 4, p, 1 << 20, p, p, p, None) == -1   # 6 m >= 2^31
    assert lib.d3d_mesh_adjacency(p, 4, 4, p, 16, p, p, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_components(None, 0, 0, None, None, None, None) == -1
    assert lib.d3d_mesh_components(p, 4, 1 << 31, p, p, ctypes.byref(rounds), None) == -1
    assert lib.d3d_mesh_component_stats(None, 0, None, 0, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.d3d_mesh_component_stats(p, 4, p, 4, p, p, 8, p, p, p, p, p, None) == -1   # scratch too small
    assert lib.d3d_mesh_filter(None, 0, 0, None, None, None, None, 0, 0.0, None, 0, None, None, None, None) == -1
    assert lib.d3d_mesh_filter(p, 4, 4, p, p, p, p, -1, 0.0, p, 1 << 20, p, p, p, None) == -1
    assert b"min_faces" in lib.d3d_last_error()
    assert lib.d3d_mesh_filter(p, 4, 4, p, p, p, p, 0, float("nan"), p, 1 << 20, p, p, p, None) == -1
    assert lib.d3d_mesh_smooth(None, 0, None, None, None, 0.5, 1, None, None, None) == -1
    assert lib.d3d_mesh_smooth(p, 4, p, p, p, 0.0, 1, ctypes.c_void_p(16), ctypes.c_void_p(24), None) == -1
    assert b"lambda" in lib.d3d_last_error()
    assert lib.d3d_mesh_smooth(p, 4, p, p, p, 0.5, -1, ctypes.c_void_p(16), ctypes.c_void_p(24), None) == -1
    assert lib.d3d_mesh_smooth(p, 4, p, p, p, 0.5, 1, p, ctypes.c_void_p(24), None) == -1   # work aliases the input
    assert lib.d3d_mesh_adjacency_scratch_bytes(-1, 0) == 0 and lib.d3d_mesh_adjacency_scratch_bytes(10, 1 << 29) == 0
    assert lib.d3d_mesh_adjacency_scratch_bytes(10, 10) > 4 * 60
    assert lib.d3d_mesh_stats_scratch_bytes(-1) == 0 and lib.d3d_mesh_stats_scratch_bytes(10) >= 10 * 28
    assert lib.d3d_mesh_filter_scratch_bytes(-1) == 0 and lib.d3d_mesh_filter_scratch_bytes(10) >= 80
