"""A mesh to collapse over mesh_refine_scene / pipeline_scene's seven 96 x 128 views of one tilted plane, for
tests/test_mesh_collapse.py and tests/test_mesh_collapse_gpu.py.

A pixel is about 3.35 world units on the plane (z about 600) and 2.7 to 2.9 at z = 520; MIN_EDGE is 1 pixel and MAX_EDGE 4.  The
pieces are disjoint, and `cases` names them by their vertex indices:
* "grid": 12 x 12 vertices with 1-unit spacing on the true plane.  Hundreds of short interior edges over several workgroups of
  the kernel, a fixed boundary that interior edges collapse onto, and boundary-boundary short edges that must stay;
* "fan": 40 faces around one vertex on the plane, the rim of radius 2 (rim spacing about 0.3 units).  The centre's row has 40
  neighbours (the adjacency's slow path, long row walks in the kernel) and 40 valid candidates that all claim it;
* hand-built pieces at z = 520 with dyadic coordinates:
  - "flip": a free vertex a with a non-convex ring; moving a onto its ring vertex b turns the face (a, r0, r1) over, so the
    short edge a-b fails test 3 (and only that).  The other spokes of a are short too, and the shortest one is valid;
  - "three": a short edge a-b whose ends share three neighbours (test 1), every other edge of the piece longer than a pixel: it
    comes back unchanged;
  - "tetra": a closed tetrahedron with unit edges (test 2): unchanged;
  - "needle_far": a short edge between two free vertices whose other neighbours are 16 units away, about 6 pixels: the guard
    (test 4) refuses it; "needle_near": the same with the neighbours 9 units away, about 3.4 pixels: it collapses to the midpoint.
    Both comparisons are tens of per cent from equality;
  - "equal": two copies of needle_near laid out fronto-parallel to the view in which their edge is longest (no view of this scene
    is fronto-parallel to z = 520), the second translated along that view's image rows.  Equality of the two measures cannot be
    reached in fp64: the translated positions round to fp32, which moves l2 by parts in 10^5, far above an fp64 ulp.  The
    translation distance is searched instead (equal_pair_frame) so that fp32(measure), the part of the measure the key holds, has
    the same bits in both: the two keys differ in their hash alone.  The CPU test asserts that, and that the fp64 values differ;
* "hidden": a hexagonal fan with unit spokes 40 units behind the plane (every view that contains it sees the plane in front),
  and "outside": the same fan outside every image.  Their measure is 0, so they are left alone, free centre and all;
* "unreferenced": a vertex no face uses.

Run as a script it is one rank of a torch.distributed.run launch over pipeline_scene's block with the mesh stage and the collapse
on:
    python -m torch.distributed.run --nproc-per-node 2 tests/mesh_collapse_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <min_edge>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_refine_scene as RS  # noqa: E402
import pipeline_scene as PS  # noqa: E402

MIN_EDGE = 1.0
MAX_EDGE = 4.0
ROUNDS = 64
TOLERANCE = 0.01
GRID_N = 12
FAN = 40
Z_HAND = 520.0
FAR, NEAR = 16.0, 9.0


def numpy_views(scene=None):
    """The views as the numpy restatement takes them: dicts with K, E, depth (and confidence)."""
    return RS.numpy_views(scene or PS.SceneViews())


class _Builder(object):
    def __init__(self):
        self.V, self.F, self.cases = [], [], {}

    def vertices(self, pts):
        first = len(self.V)
        self.V.extend([float(c) for c in p] for p in pts)
        return list(range(first, len(self.V)))

    def faces(self, tris):
        self.F.extend([int(a), int(b), int(c)] for a, b, c in tris)


def _on_plane(x, y, dz=0.0):
    return (x, y, RS.plane_z(x, y) + dz)


def _hand(B, pts, origin):
    """The planar points pts at z = Z_HAND, moved by origin."""
    return B.vertices([(origin[0] + x, origin[1] + y, Z_HAND) for x, y in pts])


def _fan(B, centre, radius, k, place):
    """k faces around centre, the rim a regular k-gon: (centre index, rim indices)."""
    ang = 2.0 * np.pi * np.arange(k) / k
    c, = B.vertices([place(centre[0], centre[1])])
    rim = B.vertices([place(centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)) for a in ang])
    B.faces([(c, rim[i], rim[(i + 1) % k]) for i in range(k)])
    return c, rim


def _needle(B, origin, ring, ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0)):
    """A unit edge a-b between two free vertices whose other neighbours lie `ring` away, in the plane through origin [3] that
    ex and ey span: (a, b, the four others)."""
    o, ex, ey = (np.asarray(x, np.float64) for x in (origin, ex, ey))
    pts = [(0.0, 0.0), (1.0, 0.0), (0.5, -ring), (0.5, ring), (-ring, 0.0), (1.0 + ring, 0.0)]
    a, b, c1, c2, l, r = B.vertices([o + x * ex + y * ey for x, y in pts])
    B.faces([(a, c1, b), (a, b, c2), (a, l, c1), (a, c2, l), (b, c1, r), (b, r, c2)])
    return a, b, (c1, c2, l, r)


def edge_l2(view, Xa, Xb):
    """l2 of the edge between the fp32 roundings of Xa and Xb in one view, by the arithmetic of §4.23's rule 3 in Python
    floats (the seen test left out)."""
    K, E = view["K"].astype(np.float64).tolist(), view["E"].astype(np.float64).tolist()
    uv = []
    for X in (Xa, Xb):
        X = np.asarray(X, np.float64).astype(np.float32).astype(np.float64).tolist()
        p = [((E[r][0] * X[0] + E[r][1] * X[1]) + E[r][2] * X[2]) + E[r][3] for r in range(3)]
        q = [(K[r][0] * p[0] + K[r][1] * p[1]) + K[r][2] * p[2] for r in range(3)]
        uv.append((q[0] / q[2], q[1] / q[2]))
    du, dv = uv[0][0] - uv[1][0], uv[0][1] - uv[1][1]
    return du * du + dv * dv


def equal_pair_frame(views, origin):
    """(k, ex, ey, D): the view k in which a unit edge at origin along the view's own image rows is longest, that view's row and
    column directions, and the distance D along the rows, the first of 24, 24 + 1/256, .. at which the translated edge has the
    same fp32(l2) in view k as the edge at origin (the distance of the nearest fp64 l2 when none has)."""
    o = np.asarray(origin, np.float64)
    k = max(range(len(views)), key=lambda i: edge_l2(views[i], o, o + views[i]["E"].astype(np.float64)[0, :3]))
    ex, ey = views[k]["E"].astype(np.float64)[0, :3], views[k]["E"].astype(np.float64)[1, :3]
    want = edge_l2(views[k], o, o + ex)
    best = None
    for j in range(8192):
        D = 24.0 + j / 256.0
        got = edge_l2(views[k], o + D * ex, o + (D + 1.0) * ex)
        if np.float32(got) == np.float32(want):
            return k, ex, ey, D
        if best is None or abs(got - want) < best[0]:
            best = (abs(got - want), D)
    return k, ex, ey, best[1]


def build(views=None):
    """(V [n, 3] fp32, F [m, 3] int32, cases): cases names the crafted pieces by their vertex indices."""
    views = views or numpy_views()
    B = _Builder()
    # the fine grid on the true plane
    gx, gy = np.meshgrid(np.arange(GRID_N) - 100.0, np.arange(GRID_N) - 80.0)
    grid = np.array(B.vertices([_on_plane(x, y) for x, y in zip(gx.ravel(), gy.ravel())])).reshape(GRID_N, GRID_N)
    for j in range(GRID_N - 1):
        for i in range(GRID_N - 1):
            a, b, c, d = grid[j, i], grid[j, i + 1], grid[j + 1, i], grid[j + 1, i + 1]
            B.faces([(a, c, b), (b, c, d)])
    B.cases["grid"] = grid
    # the fan of 40
    B.cases["fan"] = _fan(B, (-60.0, -75.0), 2.0, FAN, _on_plane)
    # test 3: a -> b turns (a, r0, r1) over
    a, r0, r1, b, r3, r4 = _hand(B, [(0, 0), (2, -1), (0.5, 0.25), (0.25, 1.5), (-1.5, 0.5), (-1, -1.5)], (-30.0, -75.0))
    B.faces([(a, r0, r1), (a, r1, b), (a, b, r3), (a, r3, r4), (a, r4, r0)])
    B.cases["flip"] = {"a": a, "b": b, "r0": r0, "r1": r1, "ring": (r0, r1, b, r3, r4)}
    # test 1: a and b share c1, c2 and c3
    a, b, c1, c2, c3, l1, l2 = _hand(B, [(0, 0), (1, 0), (0.5, -5), (0.5, 5), (0.5, 10), (-5, -5), (-5, 5)], (0.0, -75.0))
    B.faces([(a, c1, b), (a, b, c2), (a, c2, c3), (c2, b, c3), (a, l1, c1), (a, l2, l1), (a, c3, l2)])
    B.cases["three"] = {"a": a, "b": b, "all": (a, b, c1, c2, c3, l1, l2)}
    # test 2: a closed tetrahedron
    t = B.vertices([(30.0, -75.0, Z_HAND), (31.0, -75.0, Z_HAND), (30.0, -74.0, Z_HAND), (30.0, -75.0, Z_HAND - 1.0)])
    B.faces([(t[0], t[1], t[2]), (t[0], t[3], t[1]), (t[1], t[3], t[2]), (t[2], t[3], t[0])])
    B.cases["tetra"] = tuple(t)
    # test 4: the guard refuses the far needle and passes the near one
    B.cases["needle_far"] = _needle(B, (-80.0, -20.0, Z_HAND), FAR)
    B.cases["needle_near"] = _needle(B, (-30.0, -20.0, Z_HAND), NEAR)
    # two copies of the near needle fronto-parallel to the view that sees their edge longest, the second moved along its image rows
    o = np.array([20.0, -20.0, Z_HAND])
    k, ex, ey, D = equal_pair_frame(views, o)
    B.cases["equal"] = (_needle(B, o, NEAR, ex, ey), _needle(B, o + D * ex, NEAR, ex, ey), k)
    # measure 0: behind the plane, and outside every image
    B.cases["hidden"] = _fan(B, (60.0, 60.0), 1.0, 6, lambda x, y: _on_plane(x, y, 40.0))
    B.cases["outside"] = _fan(B, (-4000.0, -100.0), 1.0, 6, _on_plane)
    B.cases["unreferenced"] = B.vertices([(10.0, 10.0, 500.0)])[0]
    return np.array(B.V, np.float64).astype(np.float32), np.array(B.F, np.int32), B.cases


def main(out_dir, border, voxel, min_edge):
    import torch

    import mesh_scene as MS
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = PS.SceneViews()
    tm = {}
    mesh = dict(MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel, views_per_batch=3),
                collapse={"min_edge": min_edge, "rounds": 4})
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm, mesh=mesh)
    if rank == 0:
        print("rank %d/%d mesh_collapse %.3f s" % (rank, world, tm["mesh_collapse_s"]))
    else:
        print("rank %d/%d" % (rank, world))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), float(sys.argv[4]))
