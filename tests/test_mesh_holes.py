"""Hole closing without a GPU: a numpy restatement of rules 2-7 of deep3d_aerial_amd/mesh.py (boundary
half-edges, simple vertices, boundary components, the loop sums, which loops qualify, the output), written from the docstring;
hand cases; the properties the rule promises on the hand cases and on the numpy meshes of the scenes of tests/mesh_scene.py; the
setting and the flags of predict and of the mesh command line; the new entry points refusing null pointers and bad sizes before
any launch.  tests/test_mesh_holes_gpu.py holds the kernels to this restatement bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import test_mesh as TM
import test_mesh_clean as C
from deep3d_aerial_amd import _lib, mesh


# ----------------------------------------------------------------------------------------
# the numpy restatement
# ----------------------------------------------------------------------------------------
def boundary_numpy(n, faces):
    """Rules 2-3: boundary [m,3] uint8, out, in, successor, owner [n] int32."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = f.shape[0]
    tail, head = f.ravel(), f[:, [1, 2, 0]].ravel()
    fid = np.repeat(np.arange(m), 3)
    key = np.minimum(tail, head) * max(n, 1) + np.maximum(tail, head)
    _, inverse, holders = np.unique(key, return_inverse=True, return_counts=True)   # a face holds an undirected edge once
    b = holders[inverse] == 1 if m else np.zeros(0, bool)
    out = np.bincount(tail[b], minlength=n).astype(np.int32)
    inn = np.bincount(head[b], minlength=n).astype(np.int32)
    successor = np.full(n, -1, np.int32)
    owner = np.full(n, -1, np.int32)
    one = b & (out[tail] == 1) if m else b
    successor[tail[one]] = head[one]
    owner[tail[one]] = fid[one]
    return {"boundary": b.astype(np.uint8).reshape(m, 3), "out": out, "in": inn, "successor": successor, "owner": owner}


def loops_numpy(n, faces, d):
    """Rule 4: label [n], count and bad at the labels."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    b = d["boundary"].ravel() != 0
    tail, head = f.ravel()[b], f[:, [1, 2, 0]].ravel()[b]
    _, comp = connected_components(coo_matrix((np.ones(len(tail)), (tail, head)), shape=(n, n)), directed=False)
    mins = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(mins, comp, np.arange(n))
    label = mins[comp].astype(np.int32)
    count = np.bincount(label[tail], minlength=n).astype(np.int32)
    on = (d["out"] != 0) | (d["in"] != 0)
    simple = (d["out"] == 1) & (d["in"] == 1)
    bad = np.zeros(n, np.int32)
    bad[label[on & ~simple]] = 1
    return {"label": label, "count": count, "bad": bad}


def _cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def plan_numpy(vertices, faces, max_edges, d):
    """Rules 5-6 in Python floats (fp64, one rounding per operation): s, centroid, qualify, position, the offsets and totals."""
    x = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = x.shape[0]
    s = np.zeros(n, np.float64)
    centroid = np.zeros((n, 3), np.float32)
    qualify = np.zeros(n, np.int32)
    position = np.full(n, -1, np.int32)
    for L in np.nonzero((d["label"] == np.arange(n)) & (d["count"] >= 3) & (d["count"] <= max_edges) & (d["bad"] == 0))[0]:
        k = int(d["count"][L])
        A, N, S = [0.0] * 3, [0.0] * 3, [0.0] * 3
        a = int(L)
        for i in range(k):
            b, g = int(d["successor"][a]), int(d["owner"][a])
            xa, xb = x[a].tolist(), x[b].tolist()
            p0, p1, p2 = (x[j].tolist() for j in f[g])
            ca = _cross(xa, xb)
            cn = _cross([p1[t] - p0[t] for t in range(3)], [p2[t] - p0[t] for t in range(3)])
            for t in range(3):
                A[t] += ca[t]
                N[t] += cn[t]
                S[t] += xa[t]
            position[a] = i
            a = b
        assert a == L, "a component that is not bad is one cycle"
        s[L] = (A[0] * N[0] + A[1] * N[1]) + A[2] * N[2]
        centroid[L] = [np.float32(S[t] / float(k)) for t in range(3)]
        qualify[L] = 1 if s[L] < 0 else 0
    added = np.where(qualify != 0, d["count"], 0).astype(np.int64)
    voff = (np.cumsum(qualify) - qualify).astype(np.int32)
    foff = (np.cumsum(added) - added).astype(np.int32)
    return {"s": s, "centroid": centroid, "qualify": qualify, "position": position, "vertex_offset": voff, "face_offset": foff,
            "holes": int(qualify.sum()), "faces_added": int(added.sum())}


def close_holes_numpy(vertices, faces, max_edges):
    """(vertices, faces, detail): rule 7; detail holds every intermediate array and the info counts."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    n, m = len(v), len(f)
    d = boundary_numpy(n, f)
    d.update(loops_numpy(n, f, d))
    d.update(plan_numpy(v, f, max_edges, d))
    count, bad = d["count"], d["bad"] != 0
    small = (count >= 3) & (count <= max_edges)
    d["info"] = {"loops": int((count > 0).sum()), "holes_closed": d["holes"], "faces_added": d["faces_added"],
                 "skipped_outer": int(((count > 0) & ~bad & small).sum()) - d["holes"],
                 "skipped_large": int((~bad & (count > max_edges)).sum()), "skipped_not_simple": int(((count > 0) & bad).sum())}
    new_v = np.zeros((d["holes"], 3), np.float32)
    new_f = np.zeros((d["faces_added"], 3), np.int32)
    for L in np.nonzero(d["qualify"])[0]:
        new_v[d["vertex_offset"][L]] = d["centroid"][L]
    for a in np.nonzero(d["position"] >= 0)[0]:
        L = d["label"][a]
        if d["qualify"][L]:
            new_f[d["face_offset"][L] + d["position"][a]] = (d["successor"][a], a, n + d["vertex_offset"][L])
    return np.concatenate([v, new_v]), np.concatenate([f, new_f]), d


# ----------------------------------------------------------------------------------------
# meshes (shared with the GPU tests)
# ----------------------------------------------------------------------------------------
def grid_mesh(kx, ky=None, z=0.0):
    """kx x ky unit quads at height z, each split along its (i,j)-(i+1,j+1) diagonal, normals +z; vertex (i, j) is i + j (kx + 1)."""
    ky = kx if ky is None else ky
    j, i = np.mgrid[0:ky + 1, 0:kx + 1]
    v = np.stack([i.ravel(), j.ravel(), np.full(i.size, z)], 1).astype(np.float32)
    qj, qi = np.mgrid[0:ky, 0:kx]
    a = (qi + qj * (kx + 1)).ravel()
    b, c, d = a + 1, a + kx + 2, a + kx + 1
    f = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int32)
    return v, f


def without_fans(f, verts):
    """The faces that use none of verts."""
    return f[~np.isin(f, np.asarray(verts)).any(1)]


def annulus(k, z=0.0):
    """An inner ring (vertices 0 .. k-1, radius 1) and an outer ring (k .. 2k-1, radius 2) joined by 2 k faces, normals +z."""
    ang = np.arange(k) * 2 * np.pi / k
    ring = np.stack([np.cos(ang), np.sin(ang), np.full(k, z)], 1)
    v = np.concatenate([ring, ring * [2, 2, 1]]).astype(np.float32)
    i = np.arange(k)
    j = (i + 1) % k
    f = np.concatenate([np.stack([i, k + i, k + j], 1), np.stack([i, k + j, j], 1)]).astype(np.int32)
    return v, f


def hexagon_annulus():
    """The annulus of two hexagons with whole-number coordinates around (3, 5, 0.5): the inner loop's centroid is exact."""
    inner = np.array([[2, 0], [1, 2], [-1, 2], [-2, 0], [-1, -2], [1, -2]], np.float64)
    v = np.concatenate([inner, 2 * inner])
    v = (np.concatenate([v, np.zeros((12, 1))], 1) + [3, 5, 0.5]).astype(np.float32)
    i = np.arange(6)
    j = (i + 1) % 6
    f = np.concatenate([np.stack([i, 6 + i, 6 + j], 1), np.stack([i, 6 + j, j], 1)]).astype(np.int32)
    return v, f


def icosphere():
    """An icosahedron subdivided once on the unit sphere: 42 vertices, 80 faces, normals outward."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) for p in v]
    mid = {}

    def middle(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            mid[key] = len(v)
            v.append(v[a] + v[b])
        return mid[key]

    out = []
    for a, b, c in f:
        ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    v = np.stack(v)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), np.asarray(out, np.int32)


def _open_sphere():
    v, f = icosphere()
    return v, without_fans(f, [0])


def _bow_tie():
    """A 5 x 5 grid without the quads (1,1) and (2,2): two 4-edge holes that touch at vertex (2,2)."""
    v, f = grid_mesh(5)
    quad = lambda i, j: [2 * (i + 5 * j), 2 * (i + 5 * j) + 1]
    return v, np.delete(f, quad(1, 1) + quad(2, 2), 0)


def _three_faces_on_an_edge():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


HAND = {
    "triangle": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)),
    "hexagon_annulus": hexagon_annulus(),
    "open_tetrahedron": (C.HAND["tetrahedron"][0], C.HAND["tetrahedron"][1][1:]),
    "open_icosphere": _open_sphere(),
    "bow_tie": _bow_tie(),
    "annulus7": annulus(7, 1.25),
    "three_faces_on_an_edge": _three_faces_on_an_edge(),
    "grid_with_a_fan_removed": (grid_mesh(6, 5, 2.0)[0], without_fans(grid_mesh(6, 5, 2.0)[1], [2 + 2 * 7])),
}
SCENES = {"boxes": ("boxes", {}), "plane": ("plane", {}), "boxes_no_holes": ("boxes", {"holes": False})}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(vertices, faces) of the numpy mesh of a scene of tests/mesh_scene.py (tests/test_mesh.py's restatement), computed once."""
    which, kw = SCENES[name]
    w = TM.scene_mesh(which, **kw)[3]
    v, f = np.ascontiguousarray(w["vertices"], np.float32), np.ascontiguousarray(w["faces"], np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def case(name):
    return HAND[name] if name in HAND else scene(name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def boundary_edge_count(f):
    p = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), 1)
    return int((np.unique(p, axis=0, return_counts=True)[1] == 1).sum())


def euler(f):
    """V - E + F over the vertices some face uses."""
    p = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), 1)
    return len(np.unique(f)) - len(np.unique(p, axis=0)) + len(f)


def face_set(f):
    return set(map(tuple, np.asarray(f).tolist()))


def check_properties(v, f, max_edges):
    """What the rule promises of one call; returns (vertices, faces, detail)."""
    v2, f2, d = close_holes_numpy(v, f, max_edges)
    n, m, info = len(v), len(f), d["info"]
    assert np.array_equal(_bits(v2[:n]), _bits(v)) and np.array_equal(f2[:m], f)
    assert len(v2) == n + info["holes_closed"] and len(f2) == m + info["faces_added"]
    try:
        TM.check_manifold(f)
        manifold = True
    except AssertionError:
        manifold = False
    if manifold:
        TM.check_manifold(f2)
    closed_k = int(d["count"][d["qualify"] != 0].sum())
    assert closed_k == info["faces_added"]
    assert boundary_edge_count(f) - boundary_edge_count(f2) == closed_k
    d2 = close_holes_numpy(v2, f2, max_edges)[2]
    assert info["loops"] - d2["info"]["loops"] == info["holes_closed"]
    assert euler(f2) - euler(f) == info["holes_closed"]
    assert d2["info"]["holes_closed"] == 0 and d2["info"]["faces_added"] == 0      # a second pass closes nothing
    assert info["loops"] == info["holes_closed"] + info["skipped_outer"] + info["skipped_large"] + info["skipped_not_simple"]
    perm = np.random.default_rng(5).permutation(m)
    v3, f3, _ = close_holes_numpy(v, f[perm], max_edges)
    assert np.array_equal(_bits(v3), _bits(v2)) and face_set(f3) == face_set(f2) and len(f3) == len(f2)
    return v2, f2, d


# ----------------------------------------------------------------------------------------
# hand cases
# ----------------------------------------------------------------------------------------
def test_single_triangle_is_one_outer_loop_and_nothing_closes():
    v, f = HAND["triangle"]
    v2, f2, d = close_holes_numpy(v, f, 30)
    assert d["boundary"].all() and d["count"].tolist() == [3, 0, 0] and d["bad"].tolist() == [0, 0, 0]
    assert d["successor"].tolist() == [1, 2, 0] and d["owner"].tolist() == [0, 0, 0]
    assert d["s"][0] > 0 and d["info"]["skipped_outer"] == 1 and len(v2) == 3 and len(f2) == 1


def test_hexagon_annulus_gets_six_faces_around_the_exact_centroid_and_the_outer_loop_stays():
    v, f = HAND["hexagon_annulus"]
    for max_edges in (6, 30, mesh.HOLE_MAX_EDGES):
        v2, f2, d = close_holes_numpy(v, f, max_edges)
        assert d["info"] == {"loops": 2, "holes_closed": 1, "faces_added": 6, "skipped_outer": 1, "skipped_large": 0, "skipped_not_simple": 0}
        assert len(v2) == 13 and v2[12].tolist() == [3.0, 5.0, 0.5]
        assert d["s"][0] < 0 and d["s"][6] > 0 and d["label"].tolist() == [0] * 6 + [6] * 6
        # the inner loop runs against the ring's order (the faces lie outside it); the fan faces run with it
        assert d["successor"][:6].tolist() == [5, 0, 1, 2, 3, 4]
        assert f2[12:].tolist() == [[5, 0, 12], [4, 5, 12], [3, 4, 12], [2, 3, 12], [1, 2, 12], [0, 1, 12]]
        nz = np.cross(v2[f2[:, 1]] - v2[f2[:, 0]], v2[f2[:, 2]] - v2[f2[:, 0]])[:, 2]
        assert (nz > 0).all()                                       # the fan faces face the way the ring does
    assert close_holes_numpy(v, f, 5)[2]["info"]["skipped_large"] == 2


def test_open_tetrahedron_reads_as_an_outer_border_and_stays_open():
    v, f = HAND["open_tetrahedron"]
    v2, f2, d = close_holes_numpy(v, f, 30)
    assert d["count"][0] == 3 and d["bad"][0] == 0 and d["s"][0] == 1.0 and d["qualify"].sum() == 0
    assert len(v2) == 4 and len(f2) == 3 and d["info"]["skipped_outer"] == 1


def test_icosphere_without_one_fan_is_closed_again():
    v, f = HAND["open_icosphere"]
    assert len(f) == 75 and euler(f) == 1
    v2, f2, d = close_holes_numpy(v, f, 30)
    assert d["info"]["holes_closed"] == 1 and d["info"]["faces_added"] == 5 and euler(f2) == 2 and TM.check_manifold(f2) == 0
    ring = np.nonzero(d["out"])[0]
    assert len(ring) == 5 and np.allclose(v2[-1], v[ring].astype(np.float64).mean(0), atol=1e-6)   # the centre of the ring


def test_two_holes_touching_at_a_vertex_are_bad_and_stay_open():
    v, f = HAND["bow_tie"]
    v2, f2, d = close_holes_numpy(v, f, 30)
    touch = 2 + 2 * 6
    assert d["out"][touch] == 2 and d["in"][touch] == 2 and d["successor"][touch] == -1 and d["owner"][touch] == -1
    L = d["label"][touch]
    assert d["count"][L] == 8 and d["bad"][L] == 1 and d["info"]["skipped_not_simple"] == 1 and d["info"]["holes_closed"] == 0
    assert len(f2) == len(f)


def test_a_loop_of_max_edges_closes_and_one_edge_more_does_not():
    v, f = HAND["annulus7"]
    assert close_holes_numpy(v, f, 7)[2]["info"]["holes_closed"] == 1
    d = close_holes_numpy(v, f, 6)[2]
    assert d["info"]["holes_closed"] == 0 and d["info"]["skipped_large"] == 2 and d["s"].tolist() == [0.0] * 14
    v, f = annulus(mesh.HOLE_MAX_EDGES)
    assert close_holes_numpy(v, f, mesh.HOLE_MAX_EDGES)[2]["info"]["faces_added"] == 1024
    assert close_holes_numpy(v, f, mesh.HOLE_MAX_EDGES - 1)[2]["info"]["holes_closed"] == 0


def test_an_edge_with_three_faces_is_no_boundary_and_its_ends_are_not_simple():
    v, f = HAND["three_faces_on_an_edge"]
    v2, f2, d = close_holes_numpy(v, f, 30)
    assert d["boundary"].tolist() == [[0, 1, 1], [0, 1, 1], [0, 1, 1]]
    assert d["out"].tolist() == [1, 2, 1, 1, 1] and d["in"].tolist() == [2, 1, 1, 1, 1]
    assert d["count"][0] == 6 and d["bad"][0] == 1 and len(f2) == 3


@pytest.mark.parametrize("name", sorted(HAND) + sorted(SCENES))
def test_properties_on_hand_cases_and_scene_meshes(name):
    v, f = case(name)
    for max_edges in (30, 100) if name in SCENES else (30,):
        _, _, d = check_properties(v, f, max_edges)
        print(name, max_edges, d["info"])
        if name in SCENES:
            assert d["info"]["holes_closed"] > 0 and d["info"]["skipped_outer"] > 0


# ----------------------------------------------------------------------------------------
# settings and command lines
# ----------------------------------------------------------------------------------------
def test_close_holes_setting():
    assert mesh.HOLE_MAX_EDGES == 1024
    assert [mesh.check_close_holes_setting(k) for k in (0, 3, 30, 1024, 30.0)] == [0, 3, 30, 1024, 30]
    for bad in (-1, 2.5, 1, 2, 1025, float("nan"), "x", None):
        with pytest.raises(ValueError, match="close_holes"):
            mesh.check_close_holes_setting(bad)
    assert mesh.close_holes_setting({"path": "x", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1}) == 0   # older settings dicts: off
    assert not mesh.close_holes_requested({}) and not mesh.close_holes_requested({"close_holes": 0})
    assert mesh.close_holes_requested({"close_holes": 30}) and mesh.close_holes_setting({"close_holes": 30}) == 30
    with pytest.raises(ValueError, match="close_holes"):
        mesh.close_holes_setting({"close_holes": 2})
    assert mesh.check_clean_settings() == (0, 0.0, 0, 0.5) and mesh.clean_settings({"close_holes": 30}) == (0, 0.0, 0, 0.5)
    assert not mesh.clean_requested({"close_holes": 30})             # the clean settings keep their own tuple and meaning
    import torch

    v, f = HAND["triangle"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.close_holes(torch.from_numpy(v), torch.from_numpy(f), 30)
    with pytest.raises(ValueError, match="close_holes"):
        mesh.close_holes(torch.from_numpy(v), torch.from_numpy(f), 2)
    with pytest.raises(ValueError, match="close_holes"):
        mesh.clean(torch.from_numpy(v), torch.from_numpy(f), close_holes=1025)


def test_predict_and_mesh_command_line_flags(capsys):
    from deep3d_aerial_amd import pipeline, predict

    base = ["--model", "casmvsnet", "--loadckpt", "x.ckpt", "--data_folder", "d", "--output_folder", "o", "--fuse", "--mesh", "m.ply",
            "--mesh_border", "0,1,0,1,0,1", "--mesh_voxel", "0.1"]
    s = predict._mesh_settings(predict.parse_args(base))
    assert s["close_holes"] == 0 and not mesh.close_holes_requested(s)
    s = predict._mesh_settings(predict.parse_args(base + ["--mesh_close_holes", "30"]))
    assert s["close_holes"] == 30 and mesh.close_holes_requested(s) and not mesh.clean_requested(s)
    for bad in ("-1", "1", "2", "1025", "2.5"):
        with pytest.raises(SystemExit):
            predict.parse_args(base + ["--mesh_close_holes", bad])
        assert "close_holes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--clean", "in.ply", "--out", "o.ply", "--close_holes", "2"])
    assert "close_holes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(["--mvs", "x", "--out", "o.ply", "--border", "0,1,0,1,0,1", "--voxel", "0.1", "--close_holes", "1025"])
    assert "close_holes" in capsys.readouterr().err
    with pytest.raises(ValueError, match="close_holes"):              # predict_and_fuse checks the setting before anything runs
        pipeline.predict_and_fuse(None, None, "o", mesh={"path": "m.ply", "border": [0, 1, 0, 1, 0, 1], "voxel": 0.1, "close_holes": 2})


# ----------------------------------------------------------------------------------------
# header, binding, entry points
# ----------------------------------------------------------------------------------------
NEW = ("d3d_mesh_holes_scratch_bytes", "d3d_mesh_boundary", "d3d_mesh_boundary_loops", "d3d_mesh_holes_plan", "d3d_mesh_holes_emit")


def test_header_and_binding_carry_the_new_entry_points_and_the_abi_version_stays():
    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name + "(" in text and name in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    assert "#define D3D_MESH_HOLE_MAX_EDGES %d" % mesh.HOLE_MAX_EDGES in text
    assert "mesh_holes.hip" in open(_lib.CSRC + "/Makefile").read()


def test_new_entry_points_refuse_null_pointers_bad_sizes_and_short_scratch_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(8)
    big = 1 << 20
    assert lib.d3d_mesh_boundary(None, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_mesh_boundary(None, 4, 4, p, p, p, p, p, p, p, None) == -1                       # faces may be null only when there are none
    assert lib.d3d_mesh_boundary(p, -1, 4, p, p, p, p, p, p, p, None) == -1
    assert lib.d3d_mesh_boundary(p, 1 << 29, 4, p, p, p, p, p, p, p, None) == -1                    # 6 m >= 2^31
    assert b"n_faces" in lib.d3d_last_error()
    assert lib.d3d_mesh_boundary(p, 4, 1 << 31, p, p, p, p, p, p, p, None) == -1
    rounds = ctypes.c_int(0)
    assert lib.d3d_mesh_boundary_loops(None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_mesh_boundary_loops(p, 4, 1 << 31, p, p, p, p, p, p, p, ctypes.byref(rounds), None) == -1
    assert lib.d3d_mesh_boundary_loops(p, -3, 4, p, p, p, p, p, p, p, ctypes.byref(rounds), None) == -1
    assert lib.d3d_mesh_holes_plan(None, 0, None, 0, None, None, None, None, None, 30, None, 0, None, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    for k in (0, 2, -1, 1025):
        assert lib.d3d_mesh_holes_plan(p, 4, p, 4, p, p, p, p, p, k, p, big, p, p, p, p, p, p, p, None) == -1
        assert b"max_edges" in lib.d3d_last_error()
    assert lib.d3d_mesh_holes_plan(p, 4, p, 4, p, p, p, p, p, 30, p, 16, p, p, p, p, p, p, p, None) == -1
    assert b"scratch" in lib.d3d_last_error()
    assert lib.d3d_mesh_holes_plan(p, 4, p, 1 << 29, p, p, p, p, p, 30, p, big, p, p, p, p, p, p, p, None) == -1
    assert lib.d3d_mesh_holes_emit(None, 0, None, 0, None, None, None, None, None, None, None, 0, 0, None, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    q = ctypes.c_void_p(64)
    assert lib.d3d_mesh_holes_emit(p, 4, p, 4, p, p, p, p, p, p, p, -1, 0, q, q, None) == -1
    assert lib.d3d_mesh_holes_emit(p, 4, p, 4, p, p, p, p, p, p, p, (1 << 31) - 4, 0, q, q, None) == -1   # n + holes reaches 2^31
    assert b"n_holes" in lib.d3d_last_error()
    assert lib.d3d_mesh_holes_emit(p, 4, p, 4, p, p, p, p, p, p, p, 1, (1 << 31) - 4, q, q, None) == -1   # m + added reaches 2^31
    assert lib.d3d_mesh_holes_emit(p, 4, p, 4, p, p, p, p, p, p, p, 1, 3, p, q, None) == -1               # out_vertices aliases the input
    assert b"inputs" in lib.d3d_last_error()
    assert lib.d3d_mesh_holes_scratch_bytes(-1) == 0 and lib.d3d_mesh_holes_scratch_bytes(1 << 31) == 0
    assert lib.d3d_mesh_holes_scratch_bytes(10) >= 40 + 16 + 8
