"""A mesh to subdivide over mesh_refine_scene / pipeline_scene's seven 96 x 128 views of one tilted plane, for
tests/test_mesh_subdivide.py and tests/test_mesh_subdivide_gpu.py.

A pixel is about 3.35 world units on the plane (z about 600) and about 2.9 at z = 520; MAX_EDGE is 4 pixels.  The mesh is made of
* a coarse grid on the true plane, 8 x 5 vertices: its edges project to four to six times MAX_EDGE, it has a boundary, and it
  reaches past the images on one side;
* a fin: a third face on one interior grid edge;
* a slanted patch in front of the plane, 3 x 3 vertices rising 40 units per 12 along x: parallax makes the views disagree on which
  of its edges are longer than MAX_EDGE;
* hand-built triangles at z = 520 with dyadic coordinates, one vertex set each, whose short edges (8 units) stay and whose long
  ones (15 and more) split: no edge, one edge, two edges and three edges split, each with the special edge at corner 0, 1 and 2;
  the two-edge ones come with the diagonal a-p shorter, with b-q shorter, and isosceles, so that the two diagonals tie exactly
  with the smaller index at a and at b;
* a triangle with one vertex outside every image, a triangle behind the plane (hidden from every view that contains it), a vertex
  no face uses;
* a triangle two of whose vertices are neighbouring floats next to the centre of view 1, found by a search of the fp32 lattice
  there: in that view the edge between them is tens of pixels long, and its fp32 midpoint is one of its ends.

Run as a script it is one rank of a torch.distributed.run launch over pipeline_scene's block with the mesh stage and the
subdivision on:
    python -m torch.distributed.run --nproc-per-node 2 tests/mesh_subdivide_scene.py <out_dir> <Xmin,...,Zmax> <voxel> <max_edge>
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

MAX_EDGE = 4.0
ROUNDS = 4
TOLERANCE = 0.01
GRID_NX, GRID_NY = 8, 5
Z_HAND = 520.0
SHORT, LONG = 8.0, 15.0


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

    def face(self, a, b, c, rotate=0):
        t = (a, b, c)
        self.F.append([t[rotate % 3], t[(rotate + 1) % 3], t[(rotate + 2) % 3]])
        return len(self.F) - 1


def near_centre_pair(view):
    """Two fp32 points that differ by one ulp in x, right in front of the view's centre: both inside the image, tens of pixels
    apart.  (a, b) as fp32 triples."""
    K, E = view["K"].astype(np.float64), view["E"].astype(np.float64)
    R, t = E[:3, :3], E[:3, 3]
    base = (-R.T @ t).astype(np.float32)
    h, w = view["depth"].shape
    best = None
    for k in range(-200, 201):
        for i in range(-3, 4):
            a = base.copy()
            for _ in range(abs(k)):
                a[2] = np.nextafter(a[2], np.float32(np.inf if k > 0 else -np.inf))
            for _ in range(abs(i)):
                a[0] = np.nextafter(a[0], np.float32(np.inf if i > 0 else -np.inf))
            b = a.copy()
            b[0] = np.nextafter(a[0], np.float32(np.inf))
            uv = []
            for X in (a, b):
                p = R @ X.astype(np.float64) + t
                q = K @ p
                uv.append((q[0] / q[2], q[1] / q[2], p[2], q[2]))
            if not all(p2 > 0 and q2 > 0 and 16 <= u <= w - 17 and 16 <= v <= h - 17 for u, v, p2, q2 in uv):
                continue
            l2 = (uv[0][0] - uv[1][0]) ** 2 + (uv[0][1] - uv[1][1]) ** 2
            if 100 * MAX_EDGE ** 2 < l2 and (best is None or abs(k) < best[0]):
                best = (abs(k), a, b)
    if best is None:
        raise RuntimeError("no neighbouring floats in front of the view's centre")
    return best[1], best[2]


def build(views=None):
    """(V [n, 3] fp32, F [m, 3] int32, cases): cases names the crafted pieces by their vertex or face indices."""
    views = views or numpy_views()
    B = _Builder()
    # the grid on the true plane
    xs, ys = np.linspace(RS.X_RANGE[0], RS.X_RANGE[1], GRID_NX), np.linspace(RS.Y_RANGE[0], RS.Y_RANGE[1], GRID_NY)
    gx, gy = np.meshgrid(xs, ys)
    grid = np.array(B.vertices(np.stack([gx.ravel(), gy.ravel(), RS.plane_z(gx.ravel(), gy.ravel())], 1))).reshape(GRID_NY, GRID_NX)
    for j in range(GRID_NY - 1):
        for i in range(GRID_NX - 1):
            a, b, c, d = grid[j, i], grid[j, i + 1], grid[j + 1, i], grid[j + 1, i + 1]
            B.face(a, c, b)
            B.face(b, c, d)
    B.cases["grid"] = grid
    # a fin on an interior edge: three faces share it
    ga, gb = int(grid[2, 4]), int(grid[2, 5])
    mx, my = 0.5 * (gx[2, 4] + gx[2, 5]), gy[2, 4]
    fin, = B.vertices([(mx, my, RS.plane_z(mx, my) - 30.0)])
    B.face(ga, gb, fin)
    B.cases["three_faces"] = (ga, gb)
    # the slanted patch
    px, py = np.meshgrid(np.arange(3) * 12.0 + 28.0, np.arange(3) * 12.0 + 48.0)
    pz = RS.plane_z(40.0, 60.0) - 120.0 + (px - 28.0) * (40.0 / 12.0)
    patch = np.array(B.vertices(np.stack([px.ravel(), py.ravel(), pz.ravel()], 1))).reshape(3, 3)
    for j in range(2):
        for i in range(2):
            a, b, c, d = patch[j, i], patch[j, i + 1], patch[j + 1, i], patch[j + 1, i + 1]
            B.face(a, c, b)
            B.face(b, c, d)
    B.cases["slanted"] = patch
    # hand-built triangles: (name, (a, b, c) in the plane z = Z_HAND with the special edge a-b, swap the indices of a and b)
    h3 = 13.0
    shapes = [("none", ((0, 0), (SHORT, 0), (4, 7)), False), ("one", ((0, 0), (LONG, 0), (7.5, 3)), False),
              ("two_ap", ((-4, 0), (4, 0), (-2, 16)), False), ("two_bq", ((-4, 0), (4, 0), (2, 16)), False),
              ("two_tie_a", ((-4, 0), (4, 0), (0, 16)), False), ("two_tie_b", ((-4, 0), (4, 0), (0, 16)), True),
              ("three", ((0, 0), (LONG, 0), (7.5, h3)), False)]
    hand = {}
    for k, (name, tri, swap) in enumerate(shapes):
        for rot in range(3):
            ox, oy = -70.0 + 24.0 * k, -80.0 + 24.0 * rot
            pts = [(ox + x, oy + y, Z_HAND) for x, y in tri]
            if swap:
                ib, ia, ic = B.vertices([pts[1], pts[0], pts[2]])
            else:
                ia, ib, ic = B.vertices(pts)
            # corner `rot` of the stored face is a: edge e_rot is the special one
            hand[(name, rot)] = B.face(ia, ib, ic, rotate=-rot)
    B.cases["hand"] = hand
    # one end outside every image
    z = lambda x, y: RS.plane_z(x, y)
    out = B.vertices([(-200.0, -100.0, z(-200.0, -100.0)), (-4000.0, -100.0, z(-4000.0, -100.0)), (-200.0, -60.0, z(-200.0, -60.0))])
    B.face(*out)
    B.cases["outside"] = (out[0], out[1])
    # behind the plane: every view that contains it sees the plane in front of it
    hid = B.vertices([(0.0, 80.0, z(0.0, 80.0) + 40.0), (30.0, 80.0, z(30.0, 80.0) + 40.0), (15.0, 100.0, z(15.0, 100.0) + 40.0)])
    B.face(*hid)
    B.cases["hidden"] = (hid[0], hid[1])
    # neighbouring floats in front of view 1's centre, and a far third corner
    a, b = near_centre_pair(views[1])
    near = B.vertices([a, b, (60.0, 10.0, 300.0)])
    B.face(*near)
    B.cases["coincide"] = (near[0], near[1])
    B.cases["unreferenced"] = B.vertices([(10.0, 10.0, 500.0)])[0]
    V = np.array(B.V, np.float64).astype(np.float32)
    V[near[0]], V[near[1]] = a, b   # bit for bit
    return V, np.array(B.F, np.int32), B.cases


def core_faces(V, F, cases):
    """The faces well inside every image's reach and without the neighbouring floats: on them the loop comes to rest within ROUNDS
    rounds.  (On the whole scene it does not: an edge with an end no view sees is not measured, so along the images' border every
    round uncovers a few new long edges, and next to a camera's centre no edge ever gets short.)"""
    inside = (np.abs(V[:, 0]) <= 150.0) & (np.abs(V[:, 1]) <= 100.0)
    near = cases["coincide"][0]
    return F[[k for k, f in enumerate(F.tolist()) if near not in f and inside[f].all()]]


def main(out_dir, border, voxel, max_edge):
    import torch

    import mesh_scene as MS
    from deep3d_aerial_amd import pipeline, sharding

    rank, world = sharding.init_from_env()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    scene = PS.SceneViews()
    tm = {}
    mesh = dict(MS.pipeline_settings(os.path.join(out_dir, "mesh.ply"), border, voxel, views_per_batch=3),
                subdivide={"max_edge": max_edge, "rounds": 2})
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, os.path.join(out_dir, "MVS"), rank, world, checker=PS.checker(),
                              fusion_num=PS.FUSION_NUM, min_geo_consist_num=3, filter_sources=False, timings=tm, mesh=mesh)
    if rank == 0:
        print("rank %d/%d mesh_subdivide %.3f s" % (rank, world, tm["mesh_subdivide_s"]))
    else:
        print("rank %d/%d" % (rank, world))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], [float(v) for v in sys.argv[2].split(",")], float(sys.argv[3]), float(sys.argv[4]))
