"""Surface mesh from the depth maps.

The reference makes its mesh with OpenMVS binaries (Delaunay plus graph cut) that read a .mvs scene this project does not write,
so the mesh is this project's own: a truncated signed distance field (TSDF) of every view's depth map in sparse bricks of 8^3
voxels, and its zero surface by marching tetrahedra.

* Grid.  border [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax] (all six required) and an isotropic voxel size s.  Per axis
  n = int((max - min + 1e-8) / s), as in DsmGrid.  Voxel (i, j, k) is centred at (Xmin + (i + .5) s, Ymin + (j + .5) s,
  Zmin + (k + .5) s) in fp64.  Bricks are 8^3 voxels, ceil(n / 8) per axis; a brick at the grid's edge is partial (its voxels
  outside the grid do not exist).  A grid whose brick count (with a one-brick border) does not fit in int32 is refused.
* Views.  K [3,3] with K[1,0] = K[2,0] = K[2,1] = 0 and K[2,2] = 1, E = Tcw [4,4] (the fp32 `outcam`, used in fp64), depth and
  confidence [H,W] fp32.  A pixel is valid when its depth D is finite and > 0 and its confidence >= conf_threshold (default
  0.2, the reference's FUSION photomatric_threshold).
* Allocation.  The centre of valid pixel (x, y) is back-projected in fp64 with no contraction: yn = (y - K12) / K11,
  xn = ((x - K02) - K01 yn) / K00, c = (xn D - t0, yn D - t1, D - t2), X_a = R0a c0 + R1a c1 + R2a c2 (left to right).  Its
  brick is floor(floor((X_a - min_a) / s) / 8) per axis.  The allocated set is the 3 x 3 x 3 dilation of those bricks, clipped
  to the grid, numbered in increasing order of (bk by + bj) bx + bi by a scan (no atomic append: the numbering does not depend
  on timing).  Voxels outside allocated bricks are unobserved.
* Integration, per voxel of an allocated brick and per view in the given order.  In fp64 with no contraction p = R X + t,
  q = K p, each row summed left to right (as ortho.py).  The view observes the voxel when p2 > 0, q2 > 0, the pixel
  (floor(q1 / q2 + .5), floor(q0 / q2 + .5)) is inside the image and valid, and sdf = D - p2 >= -trunc.  It adds
  d = fp32(min(1, sdf / trunc)) to the voxel's fp32 `sum` (in view order) and 1 to its int32 `n`.  The voxel's value is
  tsdf = sum / n in fp32; it is observed when n >= min_views.  Defaults trunc = 3 s (0 < trunc <= 8 s: the truncation band
  stays inside the allocated bricks), min_views = 2.  The running sums stay fp32 between calls, so the result is bit-identical
  for any views_per_batch, but not for another view order.
* Extraction.  Every voxel is the minimum corner of a cube, split into the 6 Kuhn (Freudenthal) tetrahedra around its main
  diagonal (TETS: one per axis permutation, corners c = x | y << 1 | z << 2); every cube uses the same split, so neighbouring
  cubes agree on every face.  A tetrahedron is meshed when its 4 corners are observed; a corner is inside when tsdf < 0.  An edge
  a -> b (a its lower endpoint) that crosses the surface gets the vertex X_a + t (X_b - X_a), per component in fp64 with
  t = f_a / (f_a - f_b), rounded to fp32.  The lower endpoint owns the edge; it has 7 edge types +x, +y, +z, +xy, +xz, +yz, +xyz.
  Vertices come in (brick, voxel x-fastest, edge type) order, triangles in (brick, voxel, tetrahedron, triangle) order, and
  only vertices some triangle uses are kept.  TRI, the 16-case table (bit i: tetrahedron corner i inside), orients every
  triangle so that its right-hand normal points from the inside to the outside, toward the cameras.
* File.  Binary little-endian PLY: `element vertex` with float x, y, z and `element face` with `property list uchar int
  vertex_indices` (write_ply / read_ply).

The passes are HIP kernels (csrc/mesh.hip) with no float atomics and no order-dependent integer atomics: the mesh is a function
of the views and their order alone.

Cleaning (clean(); csrc/mesh_clean.hip).  The steps are named after the reference's ReconstructMesh clean
options (fRemoveSpurious, nSmoothMesh) but the rules are this project's; they do not claim to match OpenMVS / VCG.  The input is
vertices [n,3] fp32 and faces [m,3] int32 (extract, read_ply); every index must lie in 0 .. n - 1.
* Edges and adjacency.  The edges of face (a, b, c) are the pairs (a,b), (b,c), (c,a); a pair with equal ends is skipped and an
  unordered pair counts once per face (a face (a, a, b) has the one edge {a, b}).  N(v) is the set of distinct vertices sharing an
  edge with v, in increasing index order.  An edge is manifold when exactly two faces have it; a vertex is fixed when one of its
  edges is not manifold (boundary or non-manifold), or when it has no neighbour.
* Components.  Faces connect through shared vertices; a vertex no face uses is a component of its own.  A component's label is
  its smallest vertex index.  Per component: its face count, the fp32 box of its vertices and the box diagonal, in fp64 from the
  fp32 box: sqrt((dx dx + dy dy) + dz dz).
* Removal (min_faces > 0 or spurious > 0).  A component goes when min_faces > 0 and its face count is below min_faces, or when
  spurious > 0 and its diagonal is below D / spurious (fp64), D the diagonal of the box of every vertex some face uses.  The
  kept faces stay in input order and are renumbered; the kept vertices are those a kept face uses, in input order.
* Smoothing (smooth = k > 0).  k Jacobi iterations on the kept mesh, its adjacency rebuilt.  A fixed vertex stays; any other moves,
  per component in fp32 without contraction: s = the sum of x_u over N(v) added in increasing u (from 0),
  m = s / fp32(|N(v)|), x' = x + lambda (m - x), lambda = fp32(smooth_lambda) in (0, 1] (default 0.5).  Each iteration reads
  only the previous one's positions.
* Order: removal, then smoothing (the reference's order).  With every step off the input comes back unchanged.
The result is a function of the input arrays: shuffling the face list gives the same vertices bit for bit and the same set of
faces.  Integer atomics only, no float atomics.

Decimation (decimate(); csrc/mesh_decimate.hip): memoryless quadric-error edge collapse in rounds of
independent collapses, off by default.  The rule is this project's; it does not claim to match OpenMVS / VCG.  The input is
vertices [n,3] fp32 and faces [m,3] int32, every face with three distinct indices in 0 .. n - 1 (anything else is refused).  One
round is a function mesh -> mesh and no state is carried between rounds.  All arithmetic is fp64 without contraction, rounded to
fp32 only where said.
1. Face quadric.  nrm = (p1 - p0) x (p2 - p0), len = sqrt((nx nx + ny ny) + nz nz); a face contributes nothing unless len > 0;
   else (a, b, c) = nrm / len, d = -((a x0 + b y0) + c z0), w = len / 2 and q = (aa, ab, ac, ad, bb, bc, bd, cc, cd, dd), each term
   w * (u * v).
2. Vertex quadric Q_v: the sum of the quadrics of the faces at v, added in increasing face index, from 0 (face_incidence: the
   vertex -> face CSR, rows of any length).
3. Fixed vertices are adjacency()'s `fixed` flag.  A fixed vertex is never moved and never removed, so the mesh boundary comes
   through unchanged.
4. Candidates: one per undirected edge {a, b}, a < b, with a free endpoint (every edge at a free vertex is manifold).  Edges are
   numbered e = 0, 1, .. in (a, b) lexicographic order over all undirected edges; 3 m < 2^31 bounds their count.  Q = Q_a + Q_b.
   One endpoint fixed: it survives and the target x is its position.  Both free: a survives; with r = -(Q3, Q6, Q8),
   c00 = Q4 Q7 - Q5 Q5, c01 = Q1 Q7 - Q5 Q2, c02 = Q1 Q5 - Q4 Q2, det = (Q0 c00 - Q1 c01) + Q2 c02, m0 = r1 Q7 - Q5 r2,
   m1 = r1 Q5 - Q4 r2, m2 = Q1 r2 - r1 Q2 the minimiser is sx = ((r0 c00 - Q1 m0) + Q2 m1) / det,
   sy = ((Q0 m0 - r0 c01) + Q2 m2) / det, sz = ((-(Q0 m1) - Q1 m2) + r0 c02) / det (Cramer's rule).  x = s when det is finite and
   not 0 and |s - mid|^2 <= |x_b - x_a|^2 (mid = 0.5 (x_a + x_b), squared norms (dx dx + dy dy) + dz dz); otherwise the
   cheapest of x_a, x_b, mid (a later one only when strictly cheaper).  The distance test keeps near-planar regions (rank-1 A)
   from throwing vertices away; it is scale-free.  q(x) = ((x r0 + y r1) + z r2) + r3 with r_i = ((Q_i0 x + Q_i1 y) + Q_i2 z) + Q_i3
   the rows of the symmetric 4 x 4 matrix; the cost is c = q(x) if q(x) > 0 else 0, as fp32, and the survivor would take
   t = fp32(x).  key = (bits(fp32(c)) << 32) | (e * 2654435761 mod 2^32): the hash (a bijection of 32-bit words) spreads equal
   costs, on flat ground all of them 0, over the mesh instead of leaving the cheapest keys in one cluster that blocks itself.
5. A candidate is valid when (i) N(a) and N(b) share exactly two vertices (link condition), (ii) |N(a)| + |N(b)| - 4 >= 3 (the
   survivor keeps three neighbours: a closed tetrahedron comes back unchanged), (iii) for every face at a or b that does not
   hold both, the old normal dotted with the normal after the endpoint moves to t (the fp32 target, so the test sees the
   position really taken) is > 0: no flip, no face of zero area.
6. With T the target face count and K = ceil((m - T) / 2) collapses still needed, only the K valid candidates with the smallest
   keys are eligible this round.  A collapse removes exactly two faces, so the result has T or T - 1 faces unless it stalls.
7. Every eligible candidate writes its key by a 64-bit integer minimum into claim[w] for every w of {a, b} U N(a) U N(b); it
   wins when it reads its own key back from all of them.  Winners touch disjoint face sets; the smallest key always wins.
8. The survivor takes t, the other endpoint is re-indexed to it, the faces that held both are dropped, the others stay in input
   order, and vertices no face uses go (d3d_mesh_compact).  Adjacency is rebuilt for the next round.
9. Stop when m <= T, when a round has no winner (stalled: reported, not an error) or after max_rounds rounds (a cap on host round
   trips, reported when hit).  One small device-to-host read per round.
T = target_faces when given, else ceil(ratio m); ratio in (0, 1], 1 = off; giving both is an error.  The result is a function of
the input arrays (same bits run to run); integer atomics only.  Unlike cleaning it is NOT invariant under a shuffle of the face
list: the quadric sums run in face-index order and the kept faces keep their input order.
Order in build_and_write and the command line: removal, smoothing, then decimation (smoothing first takes the TSDF staircase out,
so flat areas have zero-cost edges).

Hole closing (close_holes(); csrc/mesh_holes.hip): every small boundary loop that is a hole gets a fan around
one new vertex, off by default.  Named after the reference's nCloseHoles, but the rule is this project's; it does not claim to
match OpenMVS / VCG.  All arithmetic is fp64 without contraction, rounded to fp32 only where said.
1. Input.  vertices [n,3] fp32 and faces [m,3] int32, every face with three distinct indices in 0 .. n - 1 (anything else is
   refused, as decimate refuses it).  max_edges is an integer: 0 means off, otherwise 3 <= max_edges <= HOLE_MAX_EDGES (1024)
   (any other value is a ValueError).
2. Boundary half-edges.  Face (a, b, c) has the directed edges a->b, b->c, c->a.  A directed edge is a boundary half-edge when
   exactly one face holds its undirected edge; its owner is that face.
3. Simple vertices.  out(v) and in(v) count the boundary half-edges that leave and enter v.  A vertex is simple when out = in
   = 1.  The successor of a->b is the outgoing boundary half-edge of b, when b is simple.
4. Boundary components.  Vertices are joined by boundary half-edges (a vertex on none is a component of its own, with nothing
   in it).  A component's label is its smallest vertex index.  Per component: its half-edge count k, and `bad`, set when any of
   its vertices is not simple.  A component that is not bad is one cycle.
5. Loop sums.  The cycle is walked from the half-edge whose tail is the label, following successors.  In walk order, starting
   from 0, with x_v the position of v in fp64: A += x_a x x_b (the cross product, per component u_y w_z - u_z w_y, u_z w_x -
   u_x w_z, u_x w_y - u_y w_x), N += (p1 - p0) x (p2 - p0) of the half-edge's owner face in that face's own corner order,
   S += x_a.  Then s = (A_x N_x + A_y N_y) + A_z N_z.
6. Which loops qualify.  A component qualifies when it is not bad, 3 <= k <= max_edges and s < 0.  The owner of a->b lies to the
   left of a->b seen from its normal's side, so A, twice the loop's area vector, points along the normals for the outer border
   of a piece (s > 0: never capped) and against them when the faces lie outside the loop (s < 0: a hole).  s == 0 or NaN is left
   alone.  A loop whose owning faces fold back by more than a right angle reads as an outer border and stays open: an open
   tetrahedron (three faces around an apex) is such a case.
7. Output.  The input vertices and faces come through first, unchanged and in place.  Each qualifying component adds one vertex
   fp32(S / k), the new vertices in increasing label order, and k faces (b, a, new), one per half-edge a->b, the new faces in
   (label, walk position) order.  One pass: the step is not iterated.  A result with n + holes or m + added faces at or above
   2^31 is refused.  With nothing to close the input tensors come back as they are.
The result is a function of the input arrays.  Shuffling the face list (without rotating corners) gives the same new vertices
bit for bit and the same set of faces.  A second call with the same max_edges closes nothing: every boundary edge of a closed
loop has become manifold, and no other loop has changed.  Integer atomics only, no float atomics.
Order in clean, build_and_write and the command line: removal, hole closing, smoothing (the smoothing relaxes the fans), then
decimation (a vertex on a closed hole is no longer fixed, so the collapse is free around it).

Collapse (collapse.py states the rule; csrc/mesh_collapse.hip), off by default: with --collapse PX
build_and_write collapses every edge shorter than PX pixels in every view that sees it, after the decimation and before the
subdivision.  No collapse may leave an edge estimated longer than --collapse_max_edge pixels (default 4 PX, or the subdivision's
length when both stages are on).

Flip (flip.py states the rule; csrc/mesh_flip.hip), off by default: with --flip DEG build_and_write flips every
interior edge whose flip raises the worse shape quality of its two triangles, where they meet at no more than DEG degrees, after
the collapse and before the subdivision (a flip can lengthen an edge, and the subdivision then splits it).  The stage needs no
views, so --clean IN.ply takes it too, after the decimation.

Subdivision (subdivide.py states the rule; csrc/mesh_subdivide.hip), off by default: with --subdivide PX
build_and_write splits every edge longer than PX pixels in a view that sees it, after the flip and before the refinement.
The order of the stages is removal, hole closing, smoothing, decimation, collapse, flip, subdivision, refinement.

    python -m deep3d_aerial_amd.mesh --mvs MVS_FOLDER --out mesh.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --voxel S
        [--trunc T] [--min_views 2] [--conf_threshold 0.2] [--views_per_batch N]
        [--min_faces N] [--spurious F] [--smooth K] [--smooth_lambda L] [--close_holes N]
        [--decimate R] [--target_faces N] [--decimate_max_rounds K] [--collapse PX] [--collapse_max_edge PX2] [--collapse_rounds R]
        [--flip DEG] [--flip_rounds R] [--subdivide PX] [--subdivide_rounds R]
    python -m deep3d_aerial_amd.mesh --clean IN.ply --out OUT.ply [--min_faces N] [--spurious F] [--smooth K] [--smooth_lambda L]
        [--close_holes N] [--decimate R] [--target_faces N] [--decimate_max_rounds K] [--flip DEG] [--flip_rounds R]
"""
import argparse
import ctypes
import math
import os

import numpy as np
import torch

from . import _geom, _lib
from ._geom import batches as _batches, ptr as _ptr, stream as _stream

DEFAULT_CONF = 0.2
DEFAULT_MIN_VIEWS = 2
DEFAULT_SMOOTH_LAMBDA = 0.5
DEFAULT_DECIMATE_MAX_ROUNDS = 1000   # a cap on host round trips, far above the rounds a target needs
DECIMATE_HASH = 2654435761
HOLE_MAX_EDGES = _lib.CONSTANTS["D3D_MESH_HOLE_MAX_EDGES"]   # the longest loop close_holes walks
BRICK = 8

# the 6 Kuhn tetrahedra (positively oriented), the edges of a tetrahedron, the 16-case table (csrc/mesh.hip has the same)
TETS = ((0, 1, 3, 7), (0, 5, 1, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 6, 4, 7))
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
TRI = ((), ((0, 1, 2),), ((0, 4, 3),), ((1, 2, 4), (1, 4, 3)), ((1, 3, 5),), ((0, 5, 2), (0, 3, 5)), ((0, 4, 5), (0, 5, 1)),
       ((2, 4, 5),), ((2, 5, 4),), ((0, 1, 5), (0, 5, 4)), ((0, 5, 3), (0, 2, 5)), ((1, 5, 3),), ((1, 3, 4), (1, 4, 2)),
       ((0, 3, 4),), ((0, 2, 1),), ())
# owned edge types in output order, as the corner at their far end
TYPE_CORNER = (1, 2, 4, 3, 5, 6, 7)


_GridRecord = _lib.STRUCTS["d3d_mesh_grid_t"]   # d3d_mesh_grid_t, as include/deep3d_planesweep.h declares it
_ViewRecord = _lib.STRUCTS["d3d_mesh_view_t"]   # d3d_mesh_view_t, likewise


class MeshGrid(object):
    """The voxel grid: border [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax] and voxel size s."""

    def __init__(self, border, voxel):
        border = [float(b) for b in border]
        if len(border) != 6:
            raise ValueError("the mesh border needs all six values Xmin, Xmax, Ymin, Ymax, Zmin, Zmax (got %d)" % len(border))
        if not all(math.isfinite(b) for b in border):
            raise ValueError("border %s must be finite" % border)
        s = float(voxel)
        if not (math.isfinite(s) and s > 0):
            raise ValueError("voxel size %r must be finite and > 0" % (voxel,))
        self.border, self.voxel = border, s
        self.min = (border[0], border[2], border[4])
        self.n = tuple(int((border[2 * a + 1] - border[2 * a] + 1e-8) / s) for a in range(3))
        if min(self.n) < 1:
            raise ValueError("empty grid %d x %d x %d" % self.n)
        self.bricks = tuple(-(-n // BRICK) for n in self.n)
        bx, by, bz = self.bricks
        if (bx + 2) * (by + 2) * (bz + 2) >= 1 << 31:
            raise ValueError("grid of %d x %d x %d bricks: the brick count does not fit in int32" % self.bricks)

    @property
    def n_bricks(self):
        return self.bricks[0] * self.bricks[1] * self.bricks[2]

    def record(self):
        return _GridRecord(self.min[0], self.min[1], self.min[2], self.voxel, *(self.n + self.bricks))

    def __repr__(self):
        return "MeshGrid(border=%s, voxel=%r, size=%s)" % (self.border, self.voxel, self.n)


class MeshView(_geom.Camera):
    """One view: K [3,3], E = Tcw [4,4] (host arrays, used in fp64), depth and confidence [H,W] fp32 on the GPU."""

    def __init__(self, K, E, depth, confidence):
        from .ops import _chk

        _geom.Camera.__init__(self, K, E)
        K = self.K
        if not (K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1 and K[0, 0] != 0 and K[1, 1] != 0):
            raise ValueError("K must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]] with fx, fy != 0 (got %s)" % K.tolist())
        _chk(depth, "depth", 2)
        _chk(confidence, "confidence", 2)
        if tuple(depth.shape) != tuple(confidence.shape) or depth.device != confidence.device:
            raise ValueError("depth %s and confidence %s must have one size and one device" % (tuple(depth.shape), tuple(confidence.shape)))
        self.depth, self.confidence = depth, confidence
        self.H, self.W = (int(s) for s in depth.shape)

    def record(self):
        r = self.fill(_ViewRecord())
        r.depth, r.conf = self.depth.data_ptr(), self.confidence.data_ptr()
        return r


def _records(views, device):
    return _geom.records((_ViewRecord * len(views))(*[v.record() for v in views]), device)


def check_settings(grid, trunc=None, min_views=DEFAULT_MIN_VIEWS, conf_threshold=DEFAULT_CONF, views_per_batch=None):
    """(trunc, min_views, conf_threshold, views_per_batch) checked, trunc defaulting to 3 s."""
    trunc = 3.0 * grid.voxel if trunc is None else float(trunc)
    if not (math.isfinite(trunc) and 0 < trunc <= 8 * grid.voxel):
        raise ValueError("trunc %r must satisfy 0 < trunc <= 8 voxel (%g)" % (trunc, 8 * grid.voxel))
    if int(min_views) != min_views or int(min_views) < 1:
        raise ValueError("min_views %r must be an integer >= 1" % (min_views,))
    conf = float(conf_threshold)
    if math.isnan(conf):
        raise ValueError("conf_threshold is NaN")
    return trunc, int(min_views), conf, _geom.check_views_per_batch(views_per_batch)


def _check_views(views, device):
    views = list(views)
    if not all(isinstance(v, MeshView) for v in views):
        raise TypeError("views must be MeshView records")
    for v in views:
        if v.depth.device != device:
            raise ValueError("every view must be on %s (got %s)" % (device, v.depth.device))
    return views


def tsdf_volume(views, grid, trunc=None, conf_threshold=DEFAULT_CONF, views_per_batch=None, device=None):
    """The sparse TSDF: {"brick_index" [bz,by,bx] int32 (-1: not allocated), "bricks" [nb] int32 linear brick indices,
    "sum" [nb, 8, 8, 8] fp32, "count" [nb, 8, 8, 8] int32 (voxel [k, j, i] of the brick)} on the device."""
    if not isinstance(grid, MeshGrid):
        raise TypeError("grid must be a MeshGrid")
    trunc, _, conf, vpb = check_settings(grid, trunc, DEFAULT_MIN_VIEWS, conf_threshold, views_per_batch)
    if device is None:
        if not views:
            raise ValueError("no views and no device")
        device = views[0].depth.device
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the mesh is built on the GPU (no CPU fallback); got %s" % device)
    views = _check_views(views, device)
    lib = _lib.load()
    g = grid.record()
    bx, by, bz = grid.bricks
    marks = torch.zeros(((bz + 2) * (by + 2) * (bx + 2),), dtype=torch.uint8, device=device)
    batches = [(b, _records(b, device)) for b in _batches(views, vpb)]
    for batch, recs in batches:
        for v0 in range(0, len(batch), 65535):   # one launch row per view
            part = batch[v0:v0 + 65535]
            rc = lib.d3d_mesh_mark(ctypes.byref(g), ctypes.c_void_p(recs.data_ptr() + v0 * ctypes.sizeof(_ViewRecord)), len(part),
                                   max(v.W * v.H for v in part), conf, _ptr(marks), _stream())
            _lib.check(rc, "d3d_mesh_mark")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, grid.n_bricks, device=device)
    index = torch.empty((bz, by, bx), dtype=torch.int32, device=device)
    blist = torch.empty((grid.n_bricks,), dtype=torch.int32, device=device)
    nb_dev = torch.empty((1,), dtype=torch.int64, device=device)
    _lib.check(lib.d3d_mesh_bricks(ctypes.byref(g), _ptr(marks), _ptr(scratch), nbytes, _ptr(index), _ptr(blist), _ptr(nb_dev),
                                   _stream()), "d3d_mesh_bricks")
    nb = int(nb_dev.item())   # the brick count sizes the volume
    if nb * BRICK ** 3 >= 1 << 31:
        raise ValueError("%d allocated bricks: more voxels than int32 indexes" % nb)
    blist = blist[:nb]
    s = torch.zeros((nb, BRICK, BRICK, BRICK), dtype=torch.float32, device=device)
    n = torch.zeros((nb, BRICK, BRICK, BRICK), dtype=torch.int32, device=device)
    for batch, recs in (batches if nb else []):
        rc = lib.d3d_mesh_integrate(ctypes.byref(g), _ptr(blist), nb, _ptr(recs), len(batch), trunc, conf, _ptr(s), _ptr(n), _stream())
        _lib.check(rc, "d3d_mesh_integrate")
    return {"brick_index": index, "bricks": blist, "sum": s, "count": n}


def extract(volume, grid, min_views=DEFAULT_MIN_VIEWS):
    """The surface of a tsdf_volume: (vertices [n,3] fp32, faces [m,3] int32) on the device."""
    _, min_views, _, _ = check_settings(grid, None, min_views)
    lib = _lib.load()
    g = grid.record()
    index, blist, s, n = volume["brick_index"], volume["bricks"], volume["sum"], volume["count"]
    dev = s.device
    nb = int(blist.shape[0])
    if nb == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    nvox = nb * BRICK ** 3
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, nvox, device=dev)
    edges = torch.empty((max(nvox, 1),), dtype=torch.uint8, device=dev)
    vbase = torch.empty((max(nvox, 1),), dtype=torch.int32, device=dev)
    fbase = torch.empty((max(nvox, 1),), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_count(ctypes.byref(g), _ptr(blist), _ptr(index), nb, _ptr(s), _ptr(n), min_views, _ptr(scratch), nbytes,
                                  _ptr(edges), _ptr(vbase), _ptr(fbase), _ptr(totals), _stream()), "d3d_mesh_count")
    nv, nf = (int(x) for x in totals.cpu())   # the counts size the outputs
    if nv >= 1 << 31 or nf >= 1 << 31:
        raise ValueError("%d vertices, %d triangles: more than int32 indexes" % (nv, nf))
    verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
    faces = torch.empty((max(nf, 1), 3), dtype=torch.int32, device=dev)
    ref = torch.zeros((max(nv, 1),), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_mesh_emit(ctypes.byref(g), _ptr(blist), _ptr(index), nb, _ptr(s), _ptr(n), min_views, _ptr(edges), _ptr(vbase),
                                 _ptr(fbase), _ptr(verts), _ptr(faces), _ptr(ref), _stream()), "d3d_mesh_emit")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, nv, device=dev)
    remap = torch.empty((max(nv, 1),), dtype=torch.int32, device=dev)
    out = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
    kept = torch.empty((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_compact(_ptr(verts), nv, _ptr(faces), nf, _ptr(ref), _ptr(scratch), nbytes, _ptr(remap), _ptr(out), _ptr(kept),
                                    _stream()), "d3d_mesh_compact")
    return out[:int(kept.item())], faces[:nf]


def depth_to_mesh(views, grid, trunc=None, min_views=DEFAULT_MIN_VIEWS, conf_threshold=DEFAULT_CONF, views_per_batch=None):
    """The mesh of `views` (MeshView, in this order) on `grid`: (vertices [n,3] fp32, faces [m,3] int32) on the device."""
    check_settings(grid, trunc, min_views, conf_threshold, views_per_batch)
    vol = tsdf_volume(views, grid, trunc, conf_threshold, views_per_batch)
    return extract(vol, grid, min_views)


# ----------------------------------------------------------------------------------------
# cleaning
# ----------------------------------------------------------------------------------------
def check_clean_settings(min_faces=0, spurious=0.0, smooth=0, smooth_lambda=DEFAULT_SMOOTH_LAMBDA):
    """(min_faces, spurious, smooth, smooth_lambda) checked; 0 turns a step off."""
    if int(min_faces) != min_faces or int(min_faces) < 0:
        raise ValueError("min_faces %r must be an integer >= 0" % (min_faces,))
    spurious = float(spurious)
    if not (math.isfinite(spurious) and spurious >= 0):
        raise ValueError("spurious %r must be finite and >= 0" % (spurious,))
    if int(smooth) != smooth or int(smooth) < 0:
        raise ValueError("smooth %r must be an integer >= 0" % (smooth,))
    lam = float(smooth_lambda)
    if not (0 < lam <= 1):
        raise ValueError("smooth_lambda %r must lie in (0, 1]" % (smooth_lambda,))
    return int(min_faces), spurious, int(smooth), lam


def _mesh_arrays(vertices, faces):
    return _geom.mesh_arrays(vertices, faces, 6, "cleaned")


def adjacency(faces, n_vertices):
    """The CSR of the distinct neighbours: (offset [n+1] int64, nbr [max(6 m, 1)] int32, fixed [n] uint8) on the device.  nbr is
    defined in [0, offset[n]), the rows; what lies past offset[n] is room the kernel never writes."""
    lib = _lib.load()
    n, m = int(n_vertices), int(faces.shape[0])
    dev = faces.device
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_adjacency_scratch_bytes, n, m, device=dev)
    if nbytes == 0:
        raise ValueError("%d vertices, %d faces: out of range" % (n, m))
    offset = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    nbr = torch.empty((max(6 * m, 1),), dtype=torch.int32, device=dev)
    fixed = torch.empty((max(n, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.d3d_mesh_adjacency(_ptr(faces), m, n, _ptr(scratch), nbytes, _ptr(offset), _ptr(nbr), _ptr(fixed), _stream()),
               "d3d_mesh_adjacency")
    return offset, nbr, fixed[:n]


def components(faces, n_vertices):
    """(labels [n] int32 on the device: the smallest vertex index of each vertex's component, rounds: hooking launches)."""
    lib = _lib.load()
    n, m = int(n_vertices), int(faces.shape[0])
    label = torch.empty((max(n, 1),), dtype=torch.int32, device=faces.device)
    flag = torch.zeros((1,), dtype=torch.int32, device=faces.device)
    rounds = ctypes.c_int(0)
    _lib.check(lib.d3d_mesh_components(_ptr(faces), m, n, _ptr(label), _ptr(flag), ctypes.byref(rounds), _stream()), "d3d_mesh_components")
    return label[:n], int(rounds.value)


def component_stats(vertices, faces, labels):
    """Per-label stats, indexed by label (entries of indices that are no label are 0 faces and a NaN box):
    {"face_count" [n] int32, "box" [n,6] fp32 (min x, y, z, max x, y, z), "diag" [n] fp64, "global_box" [6] fp32,
    "global_diag" [1] fp64 (the box of every vertex some face uses)} on the device."""
    lib = _lib.load()
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_stats_scratch_bytes, n, device=dev)
    out = {"face_count": torch.empty((max(n, 1),), dtype=torch.int32, device=dev),
           "box": torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev),
           "diag": torch.empty((max(n, 1),), dtype=torch.float64, device=dev),
           "global_box": torch.empty((6,), dtype=torch.float32, device=dev),
           "global_diag": torch.empty((1,), dtype=torch.float64, device=dev)}
    _lib.check(lib.d3d_mesh_component_stats(_ptr(vertices), n, _ptr(faces), m, _ptr(labels), _ptr(scratch), nbytes, _ptr(out["face_count"]),
                                            _ptr(out["box"]), _ptr(out["diag"]), _ptr(out["global_box"]), _ptr(out["global_diag"]),
                                            _stream()), "d3d_mesh_component_stats")
    for k in ("face_count", "box", "diag"):
        out[k] = out[k][:n]
    return out


def remove_components(vertices, faces, min_faces=0, spurious=0.0, info=None):
    """The removal step alone: (vertices, faces) of the kept components, compacted.  info (a dict) gets rounds and
    faces_removed."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    min_faces, spurious, _, _ = check_clean_settings(min_faces, spurious)
    lib = _lib.load()
    dev = vertices.device
    labels, rounds = components(faces, n)
    st = component_stats(vertices, faces, labels)
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_filter_scratch_bytes, m, device=dev)
    out_faces = torch.empty((max(m, 1), 3), dtype=torch.int32, device=dev)
    referenced = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    kept = torch.empty((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_filter(_ptr(faces), m, n, _ptr(labels), _ptr(st["face_count"]), _ptr(st["diag"]), _ptr(st["global_diag"]),
                                   min_faces, spurious, _ptr(scratch), nbytes, _ptr(out_faces), _ptr(referenced), _ptr(kept), _stream()),
               "d3d_mesh_filter")
    mk = int(kept.item())   # the kept face count sizes the renumbering
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, n, device=dev)
    remap = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    out_v = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    nk = torch.empty((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_compact(_ptr(vertices), n, _ptr(out_faces), mk, _ptr(referenced), _ptr(scratch), nbytes, _ptr(remap), _ptr(out_v),
                                    _ptr(nk), _stream()), "d3d_mesh_compact")
    if info is not None:
        info.update(rounds=rounds, faces_removed=m - mk)
    return out_v[:int(nk.item())], out_faces[:mk]


def smooth_vertices(vertices, faces, iterations, smooth_lambda=DEFAULT_SMOOTH_LAMBDA, csr=None):
    """The smoothing step alone: the vertices after `iterations` Jacobi iterations (faces unchanged).  csr: adjacency(faces, n)
    when the caller has it."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    _, _, iterations, lam = check_clean_settings(0, 0.0, iterations, smooth_lambda)
    if iterations == 0 or n == 0:
        return vertices.clone()
    offset, nbr, fixed = csr if csr is not None else adjacency(faces, n)
    work = torch.empty_like(vertices)
    out = torch.empty_like(vertices)
    _lib.check(_lib.load().d3d_mesh_smooth(_ptr(vertices), n, _ptr(offset), _ptr(nbr), _ptr(fixed), lam, iterations, _ptr(work), _ptr(out),
                                           _stream()), "d3d_mesh_smooth")
    return out


def clean(vertices, faces, min_faces=0, spurious=0.0, smooth=0, smooth_lambda=DEFAULT_SMOOTH_LAMBDA, info=None, close_holes=0):
    """Removal of small components (min_faces, spurious), then hole closing (close_holes = max_edges > 0), then `smooth` smoothing
    iterations, on the device: (vertices, faces).  With every step off the input tensors come back as they are.  info (a dict)
    gets the removal's rounds and faces_removed, and under "close_holes" the dict close_holes() fills."""
    max_edges = check_close_holes_setting(close_holes)
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    min_faces, spurious, smooth, lam = check_clean_settings(min_faces, spurious, smooth, smooth_lambda)
    if min_faces > 0 or spurious > 0:
        vertices, faces = remove_components(vertices, faces, min_faces, spurious, info=info)
    if max_edges > 0:
        hinfo = {}
        vertices, faces = _close_holes(vertices, faces, max_edges, info=hinfo)
        if info is not None:
            info["close_holes"] = hinfo
    if smooth > 0:
        vertices = smooth_vertices(vertices, faces, smooth, lam)
    return vertices, faces


# ----------------------------------------------------------------------------------------
# decimation
# ----------------------------------------------------------------------------------------
def check_decimate_settings(ratio=1.0, target_faces=0, max_rounds=DEFAULT_DECIMATE_MAX_ROUNDS):
    """(ratio, target_faces, max_rounds) checked; ratio 1 and target_faces 0 mean "off", giving both is an error."""
    ratio = float(ratio)
    if not (0 < ratio <= 1):
        raise ValueError("decimate ratio %r must lie in (0, 1]" % (ratio,))
    if int(target_faces) != target_faces or int(target_faces) < 0:
        raise ValueError("target_faces %r must be an integer >= 0" % (target_faces,))
    if ratio < 1 and int(target_faces) > 0:
        raise ValueError("decimate ratio %r and target_faces %r: give one of them" % (ratio, target_faces))
    if int(max_rounds) != max_rounds or int(max_rounds) < 1:
        raise ValueError("decimate max_rounds %r must be an integer >= 1" % (max_rounds,))
    return ratio, int(target_faces), int(max_rounds)


def _decimate_arrays(vertices, faces, what="decimation"):
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    if m and bool(((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])).any()):
        raise ValueError("a face has a repeated index: %s needs three distinct indices per face" % what)
    return vertices, faces, n, m


def face_incidence(faces, n_vertices):
    """The vertex -> face CSR: (face_offset [n+1] int32, face_index [3 m] int32), every row in increasing face index.  face_index
    is defined in [0, face_offset[n]): a face with a repeated or out-of-range index enters no row, so face_offset[n] < 3 m on a
    mesh that has one, and the entries past it are never written."""
    lib = _lib.load()
    n, m = int(n_vertices), int(faces.shape[0])
    dev = faces.device
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_incidence_scratch_bytes, n, m, device=dev)
    if nbytes == 0:
        raise ValueError("%d vertices, %d faces: out of range" % (n, m))
    foff = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    finc = torch.empty((max(3 * m, 1),), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_mesh_decimate_incidence(_ptr(faces), m, n, _ptr(scratch), nbytes, _ptr(foff), _ptr(finc), _stream()),
               "d3d_mesh_decimate_incidence")
    return foff, finc[:3 * m]


def vertex_quadrics(vertices, faces, incidence=None):
    """[n,10] fp64: the quadric of every vertex (rule 2).  incidence: face_incidence(faces, n) when the caller has it."""
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    foff, finc = incidence if incidence is not None else face_incidence(faces, n)
    q = torch.empty((max(n, 1), 10), dtype=torch.float64, device=vertices.device)
    _lib.check(_lib.load().d3d_mesh_decimate_quadrics(_ptr(vertices), n, _ptr(faces), m, _ptr(foff), _ptr(finc), _ptr(q), _stream()),
               "d3d_mesh_decimate_quadrics")
    return q[:n]


def decimate_round(vertices, faces, target_faces, detail=None):
    """One round (rules 1-8) toward target_faces: (vertices, faces, winners); with no winner the input tensors come back.
    detail (a dict) gets every pass's output: face_offset, face_index, quadric, offset, nbr, fixed, edges [E,2], target [E,3],
    cost [E], key [E] (-1: not valid), threshold, claim [n], win [E]."""
    lib = _lib.load()
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    k = max(0, -(-(m - int(target_faces)) // 2))
    if m == 0 or n == 0 or k == 0:
        return vertices, faces, 0
    st = _stream()
    offset, nbr, fixed = adjacency(faces, n)
    foff, finc = face_incidence(faces, n)
    quadric = vertex_quadrics(vertices, faces, (foff, finc))
    emax = 3 * m
    counts = torch.zeros((4,), dtype=torch.int64, device=dev)   # edges, winners, kept faces, kept vertices
    p_count = lambda i: ctypes.c_void_p(counts.data_ptr() + 8 * i)
    edges = torch.empty((emax, 2), dtype=torch.int32, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_edges_scratch_bytes, n, device=dev)
    _lib.check(lib.d3d_mesh_decimate_edges(_ptr(offset), _ptr(nbr), n, _ptr(scratch), nbytes, emax, _ptr(edges), p_count(0), st),
               "d3d_mesh_decimate_edges")
    target = torch.empty((emax, 3), dtype=torch.float32, device=dev)
    cost = torch.empty((emax,), dtype=torch.float32, device=dev)
    key = torch.empty((emax,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_decimate_candidates(_ptr(vertices), n, _ptr(faces), m, _ptr(offset), _ptr(nbr), _ptr(fixed), _ptr(foff), _ptr(finc),
                                                _ptr(quadric), _ptr(edges), p_count(0), emax, _ptr(target), _ptr(cost), _ptr(key), st),
               "d3d_mesh_decimate_candidates")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_select_scratch_bytes, device=dev)
    threshold = torch.empty((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_decimate_select(_ptr(key), emax, k, _ptr(scratch), nbytes, _ptr(threshold), st), "d3d_mesh_decimate_select")
    claim = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_decimate_claim(_ptr(offset), _ptr(nbr), n, _ptr(edges), _ptr(key), p_count(0), emax, _ptr(threshold), _ptr(claim),
                                           p_count(1), st), "d3d_mesh_decimate_claim")
    moved = torch.empty_like(vertices)
    remap = torch.empty((n,), dtype=torch.int32, device=dev)
    win = torch.empty((emax,), dtype=torch.uint8, device=dev)
    _lib.check(lib.d3d_mesh_decimate_apply(_ptr(vertices), n, _ptr(offset), _ptr(nbr), _ptr(fixed), _ptr(edges), _ptr(key), _ptr(target),
                                           p_count(0), emax, _ptr(threshold), _ptr(claim), _ptr(moved), _ptr(remap), _ptr(win), p_count(1), st),
               "d3d_mesh_decimate_apply")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_faces_scratch_bytes, m, device=dev)
    out_faces = torch.zeros((m, 3), dtype=torch.int32, device=dev)   # rows past the kept ones stay 0: a valid index
    referenced = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_mesh_decimate_faces(_ptr(faces), m, n, _ptr(remap), _ptr(scratch), nbytes, _ptr(out_faces), _ptr(referenced), p_count(2),
                                           st), "d3d_mesh_decimate_faces")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, n, device=dev)
    renum = torch.empty((n,), dtype=torch.int32, device=dev)
    out_v = torch.empty((n, 3), dtype=torch.float32, device=dev)
    # the kept count is still on the device, so all m rows are renumbered; the round's one read comes after
    _lib.check(lib.d3d_mesh_compact(_ptr(moved), n, _ptr(out_faces), m, _ptr(referenced), _ptr(scratch), nbytes, _ptr(renum), _ptr(out_v),
                                    p_count(3), st), "d3d_mesh_compact")
    ne, nw, mk, nk = (int(x) for x in counts.cpu())   # the round's one device-to-host read: it sizes the next round
    if detail is not None:
        detail.update(face_offset=foff, face_index=finc, quadric=quadric, offset=offset, nbr=nbr[:2 * ne], fixed=fixed, edges=edges[:ne],
                      target=target[:ne], cost=cost[:ne], key=key[:ne], threshold=threshold, claim=claim, win=win[:ne], eligible=k)
    if nw == 0:
        return vertices, faces, 0
    return out_v[:nk], out_faces[:mk], nw


def decimate(vertices, faces, ratio=1.0, target_faces=0, max_rounds=DEFAULT_DECIMATE_MAX_ROUNDS, info=None):
    """Quadric-error edge collapse toward T = target_faces (when > 0) or ceil(ratio m) faces, on the device: (vertices, faces).
    With ratio 1 and target_faces 0, or T >= m, the input tensors come back as they are.  info (a dict) gets target_faces, rounds,
    collapses (per round), faces_in, faces_out, vertices_out, stalled and hit_max_rounds."""
    ratio, target_faces, max_rounds = check_decimate_settings(ratio, target_faces, max_rounds)
    m0 = int(faces.shape[0]) if isinstance(faces, torch.Tensor) and faces.dim() == 2 else 0
    goal = target_faces if target_faces > 0 else int(math.ceil(ratio * m0))
    rec = {"target_faces": goal, "rounds": 0, "collapses": [], "faces_in": m0, "faces_out": m0, "stalled": False, "hit_max_rounds": False}
    if (ratio == 1.0 and target_faces == 0) or goal >= m0:
        _mesh_arrays(vertices, faces)
        rec["vertices_out"] = int(vertices.shape[0])
        if info is not None:
            info.update(rec)
        return vertices, faces
    v, f, n, m = _decimate_arrays(vertices, faces)
    while int(f.shape[0]) > goal:
        if rec["rounds"] >= max_rounds:
            rec["hit_max_rounds"] = True
            break
        v, f, won = decimate_round(v, f, goal)
        rec["rounds"] += 1
        rec["collapses"].append(won)
        if won == 0:
            rec["stalled"] = True
            break
    rec.update(faces_out=int(f.shape[0]), vertices_out=int(v.shape[0]))
    if info is not None:
        info.update(rec)
    return v, f


# ----------------------------------------------------------------------------------------
# hole closing
# ----------------------------------------------------------------------------------------
def check_close_holes_setting(max_edges=0):
    """max_edges checked: 0 (off) or an integer in 3 .. HOLE_MAX_EDGES."""
    try:
        whole = int(max_edges) == max_edges
    except (TypeError, ValueError):
        whole = False
    if not whole or not (int(max_edges) == 0 or 3 <= int(max_edges) <= HOLE_MAX_EDGES):
        raise ValueError("close_holes %r must be 0 (off) or an integer in 3 .. %d" % (max_edges, HOLE_MAX_EDGES))
    return int(max_edges)


def _boundary(faces, n, incidence=None):
    """d3d_mesh_boundary on checked arrays: boundary, out, in, successor, owner (full-size tensors)."""
    lib = _lib.load()
    m = int(faces.shape[0])
    dev = faces.device
    foff, finc = incidence if incidence is not None else face_incidence(faces, n)
    i32 = lambda: torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    d = {"out": i32(), "in": i32(), "successor": i32(), "owner": i32(), "boundary": torch.empty((max(3 * m, 1),), dtype=torch.uint8, device=dev)}
    _lib.check(lib.d3d_mesh_boundary(_ptr(faces), m, n, _ptr(foff), _ptr(finc), _ptr(d["out"]), _ptr(d["in"]), _ptr(d["successor"]),
                                     _ptr(d["owner"]), _ptr(d["boundary"]), _stream()), "d3d_mesh_boundary")
    return d


def _loops(faces, n, d):
    """d3d_mesh_boundary_loops on _boundary's dict: adds label, count, bad and rounds."""
    lib = _lib.load()
    m = int(faces.shape[0])
    dev = faces.device
    i32 = lambda: torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    d.update(label=i32(), count=i32(), bad=i32())
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    rounds = ctypes.c_int(0)
    _lib.check(lib.d3d_mesh_boundary_loops(_ptr(faces), m, n, _ptr(d["boundary"]), _ptr(d["out"]), _ptr(d["in"]), _ptr(d["label"]),
                                           _ptr(d["count"]), _ptr(d["bad"]), _ptr(flag), ctypes.byref(rounds), _stream()),
               "d3d_mesh_boundary_loops")
    d["rounds"] = int(rounds.value)
    return d


def _boundary_loops(faces, n, incidence=None):
    m = int(faces.shape[0])
    d = _loops(faces, n, _boundary(faces, n, incidence))
    for k in ("out", "in", "successor", "owner", "label", "count", "bad"):
        d[k] = d[k][:n]
    d["boundary"] = d["boundary"][:3 * m].view(m, 3)
    return d


def boundary_loops(faces, n_vertices):
    """The boundary of a mesh (hole closing, rules 2-4), on the device: {"boundary" [m,3] uint8 (corner c: the edge from corner c
    to the next is a boundary half-edge), "out", "in" [n] int32, "successor", "owner" [n] int32 (the head and the owning face of
    the vertex's outgoing boundary half-edge where out is 1, else -1), "label" [n] int32, "count", "bad" [n] int32 (at a label,
    0 elsewhere), "rounds": hooking launches (the one entry that may differ from run to run: a launch may or may not see a
    parent lowered in the same launch)}."""
    n = int(n_vertices)
    _, faces, _, _ = _decimate_arrays(torch.empty((n, 3), dtype=torch.float32, device=faces.device), faces, "hole closing")
    return _boundary_loops(faces, n)


def plan_holes(vertices, faces, max_edges, loops=None):
    """The loops close_holes would close (rules 5-6), on the device: boundary_loops' dict plus {"s" [n] fp64, "centroid" [n,3]
    fp32, "qualify" [n] int32 (at the label of every walked loop, 0 elsewhere), "position" [n] int32 (the walk position of the
    vertex's outgoing half-edge, -1: not walked), "vertex_offset", "face_offset" [n] int32, "holes", "faces_added": the totals}.
    One device-to-host read."""
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "hole closing")
    max_edges = check_close_holes_setting(max_edges)
    if max_edges == 0 or m == 0:
        raise ValueError("plan_holes needs faces and max_edges in 3 .. %d" % HOLE_MAX_EDGES)
    return _plan_holes(vertices, faces, n, m, max_edges, loops)


def _plan_holes(vertices, faces, n, m, max_edges, loops=None):
    lib = _lib.load()
    dev = vertices.device
    d = dict(loops) if loops is not None else _boundary_loops(faces, n)
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_holes_scratch_bytes, n, device=dev)
    i32 = lambda: torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    s = torch.empty((max(n, 1),), dtype=torch.float64, device=dev)
    centroid = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    qualify, position, voff, foff = i32(), i32(), i32(), i32()
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_holes_plan(_ptr(vertices), n, _ptr(faces), m, _ptr(d["successor"]), _ptr(d["owner"]), _ptr(d["label"]),
                                       _ptr(d["count"]), _ptr(d["bad"]), max_edges, _ptr(scratch), nbytes, _ptr(s), _ptr(centroid),
                                       _ptr(qualify), _ptr(position), _ptr(voff), _ptr(foff), _ptr(totals), _stream()), "d3d_mesh_holes_plan")
    holes, added = (int(x) for x in totals.cpu())   # the totals size the outputs
    d.update(s=s[:n], centroid=centroid[:n], qualify=qualify[:n], position=position[:n], vertex_offset=voff[:n], face_offset=foff[:n],
             holes=holes, faces_added=added)
    return d


def close_holes(vertices, faces, max_edges, info=None):
    """Closes every boundary loop of at most max_edges edges that is a hole with a fan around one new vertex, on the device:
    (vertices, faces), the input first and unchanged.  With max_edges 0, or nothing to close, the input tensors come back as they
    are.  info (a dict) gets loops (boundary components), holes_closed, faces_added, skipped_outer (walked, s not below 0),
    skipped_large (more than max_edges edges), skipped_not_simple (bad) and rounds."""
    max_edges = check_close_holes_setting(max_edges)
    if max_edges == 0:
        _mesh_arrays(vertices, faces)
        if info is not None:
            info.update(loops=0, holes_closed=0, faces_added=0, skipped_outer=0, skipped_large=0, skipped_not_simple=0, rounds=0)
        return vertices, faces
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "hole closing")
    if m == 0:
        if info is not None:
            info.update(loops=0, holes_closed=0, faces_added=0, skipped_outer=0, skipped_large=0, skipped_not_simple=0, rounds=0)
        return vertices, faces
    p = _plan_holes(vertices, faces, n, m, max_edges)
    holes, added = p["holes"], p["faces_added"]
    if info is not None:
        count, bad = p["count"], p["bad"] != 0
        small = (count >= 3) & (count <= max_edges)
        info.update(loops=int((count > 0).sum()), holes_closed=holes, faces_added=added,
                    skipped_outer=int(((count > 0) & ~bad & small).sum()) - holes, skipped_large=int((~bad & (count > max_edges)).sum()),
                    skipped_not_simple=int(((count > 0) & bad).sum()), rounds=p["rounds"])
    if holes == 0:
        return vertices, faces
    if n + holes >= 1 << 31 or m + added >= 1 << 31:
        raise ValueError("%d + %d vertices, %d + %d faces: more than int32 indexes" % (n, holes, m, added))
    out_v = torch.empty((n + holes, 3), dtype=torch.float32, device=vertices.device)
    out_f = torch.empty((m + added, 3), dtype=torch.int32, device=vertices.device)
    _lib.check(_lib.load().d3d_mesh_holes_emit(_ptr(vertices), n, _ptr(faces), m, _ptr(p["successor"]), _ptr(p["label"]), _ptr(p["qualify"]),
                                               _ptr(p["position"]), _ptr(p["vertex_offset"]), _ptr(p["face_offset"]), _ptr(p["centroid"]),
                                               holes, added, _ptr(out_v), _ptr(out_f), _stream()), "d3d_mesh_holes_emit")
    return out_v, out_f


_close_holes = close_holes   # clean() has a keyword of the same name


# ----------------------------------------------------------------------------------------
# PLY
# ----------------------------------------------------------------------------------------
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def ply_header(n_vertices, n_faces):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (n_vertices, n_faces)).encode("ascii")


def write_ply(path, vertices, faces):
    """Writes the binary little-endian PLY.  vertices [n,3] fp32, faces [m,3] int32 (tensors on any device, or arrays)."""
    if isinstance(vertices, torch.Tensor):
        vertices = vertices.detach().cpu().numpy()
    if isinstance(faces, torch.Tensor):
        faces = faces.detach().cpu().numpy()
    v = np.ascontiguousarray(vertices, "<f4").reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    rec = np.empty((f.shape[0],), FACE_DTYPE)
    rec["n"] = 3
    rec["v"] = f
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(ply_header(v.shape[0], f.shape[0]))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())
    return str(path)


def read_ply(path):
    """(vertices [n,3] float32, faces [m,3] int32) of a file write_ply wrote."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    lines = data[:end].decode("ascii").split("\n")
    counts = {}
    for ln in lines:
        w = ln.split()
        if len(w) == 3 and w[0] == "element":
            counts[w[1]] = int(w[2])
    nv, nf = counts.get("vertex"), counts.get("face")
    if nv is None or nf is None or data[:end + 11] != ply_header(nv, nf):
        raise ValueError("%s: not a PLY file write_ply wrote" % path)
    body = data[end + 11:]
    if len(body) != nv * 12 + nf * FACE_DTYPE.itemsize:
        raise ValueError("%s: %d bytes of data, %d expected" % (path, len(body), nv * 12 + nf * FACE_DTYPE.itemsize))
    v = np.frombuffer(body[:nv * 12], "<f4").reshape(nv, 3).astype(np.float32)
    rec = np.frombuffer(body[nv * 12:], FACE_DTYPE)
    if nf and not (rec["n"] == 3).all():
        raise ValueError("%s: only triangles are read" % path)
    return v, rec["v"].astype(np.int32).reshape(nf, 3)


# ----------------------------------------------------------------------------------------
# predict's products -> views; settings; command line
# ----------------------------------------------------------------------------------------
def load_mvs_views(mvs_folder, device="cuda"):
    """MeshView records of every {name}_init.pfm + {name}_prob.pfm + {name}.txt predict wrote under mvs_folder, in increasing
    order of the image id in the camera file (then name): predict's view order when the view pair file lists its reference
    views by increasing id, as it usually does."""
    views = []
    for name, cam, _, _ in sorted(_geom.mvs_cameras(mvs_folder), key=lambda r: (int(r[2][2]), r[0])):
        views.append(MeshView(cam[1, :3, :3], cam[0], _geom.load_map(mvs_folder, name, "_init", device),
                              _geom.load_map(mvs_folder, name, "_prob", device)))
    return views


def parse_border6(text):
    vals = [float(v) for v in str(text).split(",")]
    if len(vals) != 6:
        raise argparse.ArgumentTypeError("the mesh border needs Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (got %d values)" % len(vals))
    return vals


def add_arguments(ap, prefix=""):
    """The mesh settings as flags (--<prefix>border, ...); used by this module's CLI and by predict (--mesh_*)."""
    ap.add_argument("--%sborder" % prefix, type=parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--%svoxel" % prefix, type=float, default=None, help="voxel size (world units)")
    ap.add_argument("--%strunc" % prefix, type=float, default=None, help="truncation distance (default 3 voxels, at most 8)")
    ap.add_argument("--%smin_views" % prefix, type=int, default=DEFAULT_MIN_VIEWS, help="views a voxel needs to be observed")
    ap.add_argument("--%sconf_threshold" % prefix, type=float, default=DEFAULT_CONF, help="a pixel is used when its confidence >= this")
    ap.add_argument("--%sviews_per_batch" % prefix, type=int, default=None, help="views per integration call (default: all)")
    add_clean_arguments(ap, prefix)
    add_decimate_arguments(ap, prefix)
    add_collapse_arguments(ap, prefix)
    add_flip_arguments(ap, prefix)
    add_subdivide_arguments(ap, prefix)


def add_collapse_arguments(ap, prefix=""):
    """The collapse step as flags (--<prefix>collapse PX, --<prefix>collapse_max_edge PX2, --<prefix>collapse_rounds R); off unless
    PX is given."""
    from . import collapse as _collapse

    _collapse.add_arguments(ap, prefix + "collapse_", edge_flag="--%scollapse" % prefix, tolerance=False)


def add_flip_arguments(ap, prefix=""):
    """The flip step as flags (--<prefix>flip DEG, --<prefix>flip_rounds R); off unless DEG is given."""
    from . import flip as _flip

    _flip.add_arguments(ap, prefix + "flip_", angle_flag="--%sflip" % prefix)


def add_subdivide_arguments(ap, prefix=""):
    """The subdivision step as flags (--<prefix>subdivide PX, --<prefix>subdivide_rounds R); off unless PX is given."""
    from . import subdivide as _subdivide

    _subdivide.add_arguments(ap, prefix + "subdivide_", edge_flag="--%ssubdivide" % prefix, tolerance=False)


def add_decimate_arguments(ap, prefix=""):
    """The decimation step as flags (--<prefix>decimate, --<prefix>target_faces, --<prefix>decimate_max_rounds); off by default."""
    ap.add_argument("--%sdecimate" % prefix, type=float, default=1.0, metavar="R",
                    help="decimate to ceil(R m) faces by quadric-error edge collapse, R in (0, 1] (1: off)")
    ap.add_argument("--%starget_faces" % prefix, type=int, default=0, metavar="N", help="decimate to N faces instead of a ratio (0: off)")
    ap.add_argument("--%sdecimate_max_rounds" % prefix, type=int, default=DEFAULT_DECIMATE_MAX_ROUNDS, metavar="K",
                    help="cap on the collapse rounds (host round trips); reaching it is reported")


def add_clean_arguments(ap, prefix=""):
    """The clean steps as flags (--<prefix>min_faces, ...); all off by default."""
    ap.add_argument("--%smin_faces" % prefix, type=int, default=0, help="remove components of fewer faces (0: off)")
    ap.add_argument("--%sspurious" % prefix, type=float, default=0.0,
                    help="remove components whose box diagonal is below the mesh's divided by this (0: off)")
    ap.add_argument("--%ssmooth" % prefix, type=int, default=0, help="Laplacian smoothing iterations (0: off)")
    ap.add_argument("--%ssmooth_lambda" % prefix, type=float, default=DEFAULT_SMOOTH_LAMBDA, help="smoothing step in (0, 1]")
    ap.add_argument("--%sclose_holes" % prefix, type=int, default=0, metavar="N",
                    help="close the holes of at most N boundary edges, 3 .. %d, after the removal and before the smoothing (0: off)" % HOLE_MAX_EDGES)


def settings_from_args(a, path, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    s = {"path": path, "border": g("border"), "voxel": g("voxel"), "trunc": g("trunc"), "min_views": g("min_views"),
            "conf_threshold": g("conf_threshold"), "views_per_batch": g("views_per_batch"), "min_faces": g("min_faces"),
            "spurious": g("spurious"), "smooth": g("smooth"), "smooth_lambda": g("smooth_lambda"), "decimate": g("decimate"),
            "target_faces": g("target_faces"), "decimate_max_rounds": g("decimate_max_rounds"), "close_holes": g("close_holes")}
    if getattr(a, prefix + "subdivide_max_edge", None) is not None:   # the key is carried only when the flag is given
        from . import subdivide as _subdivide

        s["subdivide"] = {k: v for k, v in _subdivide.settings_from_args(a, prefix + "subdivide_").items() if k != "views_per_batch"}
    if getattr(a, prefix + "collapse_min_edge", None) is not None:   # likewise
        from . import collapse as _collapse

        s["collapse"] = {k: v for k, v in _collapse.settings_from_args(a, prefix + "collapse_").items() if k != "views_per_batch"}
    if getattr(a, prefix + "flip_max_angle", None) is not None:   # likewise
        from . import flip as _flip

        s["flip"] = _flip.settings_from_args(a, prefix + "flip_")
    return s


def clean_settings(settings):
    """(min_faces, spurious, smooth, smooth_lambda) of a settings dict, checked; missing keys mean "off"."""
    return check_clean_settings(settings.get("min_faces") or 0, settings.get("spurious") or 0.0, settings.get("smooth") or 0,
                                settings.get("smooth_lambda", DEFAULT_SMOOTH_LAMBDA))


def clean_requested(settings):
    min_faces, spurious, smooth, _ = clean_settings(settings)
    return min_faces > 0 or spurious > 0 or smooth > 0


def close_holes_setting(settings):
    """max_edges of a settings dict ("close_holes"), checked; a missing key means "off"."""
    return check_close_holes_setting(0 if settings.get("close_holes") is None else settings["close_holes"])


def close_holes_requested(settings):
    return close_holes_setting(settings) > 0


def decimate_settings(settings):
    """(ratio, target_faces, max_rounds) of a settings dict, checked; missing keys mean "off"."""
    return check_decimate_settings(1.0 if settings.get("decimate") is None else settings["decimate"], settings.get("target_faces") or 0,
                                   DEFAULT_DECIMATE_MAX_ROUNDS if settings.get("decimate_max_rounds") is None else settings["decimate_max_rounds"])


def decimate_requested(settings):
    ratio, target_faces, _ = decimate_settings(settings)
    return ratio < 1 or target_faces > 0


def subdivide_settings(settings):
    """The checked subdivision settings of a settings dict ("subdivide": {"max_edge", "rounds", "depth_tolerance"}, with the mesh
    settings' own views_per_batch), or None when the key is missing: the step is off."""
    if settings.get("subdivide") is None:
        return None
    from . import subdivide as _subdivide

    if "views_per_batch" in settings["subdivide"]:
        raise ValueError("subdivide: views_per_batch is the mesh settings' own")
    return _subdivide.check_subdivide_settings(dict(settings["subdivide"], views_per_batch=settings.get("views_per_batch")))


def collapse_settings(settings):
    """The checked collapse settings of a settings dict ("collapse": {"min_edge", "max_edge", "rounds", "depth_tolerance"}, with
    the mesh settings' own views_per_batch), or None when the key is missing: the step is off.  Without a max_edge of its own the
    collapse takes the subdivision's when that stage is on too (a ValueError when it is below 2 min_edge), else 4 min_edge."""
    if settings.get("collapse") is None:
        return None
    from . import collapse as _collapse

    if "views_per_batch" in settings["collapse"]:
        raise ValueError("collapse: views_per_batch is the mesh settings' own")
    s = dict(settings["collapse"], views_per_batch=settings.get("views_per_batch"))
    sub = subdivide_settings(settings)
    if s.get("max_edge") is None and sub is not None:
        s["max_edge"] = sub["max_edge"]
    return _collapse.check_collapse_settings(s)


def flip_settings(settings):
    """The checked flip settings of a settings dict ("flip": {"max_angle", "rounds"}), or None when the key is missing: the step is
    off."""
    if settings.get("flip") is None:
        return None
    from . import flip as _flip

    return _flip.check_flip_settings(settings["flip"])


def check_args(ap, a, prefix=""):
    """The argument errors of the mesh settings, reported through ap.error."""
    if getattr(a, prefix + "border") is None:
        ap.error("--%sborder Xmin,Xmax,Ymin,Ymax,Zmin,Zmax is required" % prefix)
    if getattr(a, prefix + "voxel") is None:
        ap.error("--%svoxel is required" % prefix)
    try:
        s = settings_from_args(a, None, prefix)
        check_settings(MeshGrid(s["border"], s["voxel"]), s["trunc"], s["min_views"], s["conf_threshold"], s["views_per_batch"])
        edit_settings(s)
    except ValueError as e:
        ap.error("--%s*: %s" % (prefix, e))


def _decimate_and_report(v, f, ratio, target_faces, max_rounds):
    info = {}
    v, f = decimate(v, f, ratio, target_faces, max_rounds, info=info)
    if info["stalled"] or info["hit_max_rounds"]:
        print("mesh decimation %s after %d rounds at %d faces (target %d)" % ("stalled" if info["stalled"] else "reached max_rounds",
                                                                              info["rounds"], info["faces_out"], info["target_faces"]))
    return v, f


def _clean_step(settings):
    """clean()'s arguments when a clean step or the hole closing is on, else None."""
    if clean_requested(settings) or close_holes_requested(settings):
        return clean_settings(settings) + (close_holes_setting(settings),)
    return None


def _decimate_step(settings):
    return decimate_settings(settings) if decimate_requested(settings) else None


# The edit steps in the order they run: key, the function that checks its settings of a settings dict (None: the step is off),
# whether it takes the views, what runs it -- a function of (vertices, faces, settings), or the (module, function) of a stage that
# fills an info dict and has a summary_line --, that stage's label, its "nothing to ..." text and its timing key.
EDIT_STEPS = (
    ("clean", _clean_step, False, lambda v, f, s: clean(v, f, *s[:4], close_holes=s[4]), None, None, None),
    ("decimate", _decimate_step, False, lambda v, f, s: _decimate_and_report(v, f, *s), None, None, None),
    ("collapse", collapse_settings, True, ("collapse", "collapse"), "mesh collapse", "nothing to collapse", "mesh_collapse_s"),
    ("flip", flip_settings, False, ("flip", "flip_edges"), "mesh flip", "nothing to flip", "mesh_flip_s"),
    ("subdivide", subdivide_settings, True, ("subdivide", "subdivide"), "mesh subdivision", "nothing to split", "mesh_subdivide_s"),
)


def edit_settings(settings):
    """Every edit step's settings of a settings dict, checked once: {key: what the step takes, or None when it is off}."""
    return {step[0]: step[1](settings) for step in EDIT_STEPS}


def _edit_and_report(v, f, views, s, step, timings=None):
    import importlib

    _, _, takes_views, (module, name), label, nothing, key = step
    stage = importlib.import_module("." + module, __package__)
    info = {}
    with _geom.timed(timings, key, start=True, always=False):
        v, f = getattr(stage, name)(v, f, *((views,) if takes_views else ()), info=info, **s)
    print("%s: %s" % (label, stage.summary_line(info) or nothing))
    return v, f


def _edit(v, f, views, steps, timings=None):
    """The edit steps that are on (steps: edit_settings' dict), in EDIT_STEPS' order: (vertices, faces)."""
    for step in EDIT_STEPS:
        s = steps[step[0]]
        if s is not None:
            v, f = step[3](v, f, s) if callable(step[3]) else _edit_and_report(v, f, views, s, step, timings)
    return v, f


def build_and_write(views, settings, refine=None, timings=None):
    """depth_to_mesh with the settings dict (settings_from_args), then the edit steps that are on, in EDIT_STEPS' order: clean when a
    clean step is on (removal, hole closing, smoothing), decimate when it is on, collapse the edges `views` cannot resolve when
    settings["collapse"] is present (collapse.collapse; timings, a dict, then gets mesh_collapse_s), flip the edges whose flip
    removes a cap triangle when settings["flip"] is present (flip.flip_edges; timings then gets mesh_flip_s), subdivide against
    `views` when settings["subdivide"] is present (subdivide.subdivide; timings then gets mesh_subdivide_s); then vertices =
    refine(vertices, faces) when a refinement is handed in (refine.refine_mesh bound to its views: pipeline.write_mesh_of), and
    write_ply to settings["path"]: (vertices, faces) as written."""
    steps = edit_settings(settings)
    grid = MeshGrid(settings["border"], settings["voxel"])
    v, f = depth_to_mesh(views, grid, settings.get("trunc"), settings.get("min_views", DEFAULT_MIN_VIEWS),
                         settings.get("conf_threshold", DEFAULT_CONF), settings.get("views_per_batch"))
    v, f = _edit(v, f, views, steps, timings)
    if refine is not None:
        v = refine(v, f)
    write_ply(settings["path"], v, f)
    return v, f


def main(argv=None):
    ap = argparse.ArgumentParser(description="surface mesh (binary PLY) from predict's depth maps, confidences and cameras; or --clean "
                                             "an existing mesh")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--mvs", help="predict's output folder: {name}_init.pfm, {name}_prob.pfm and {name}.txt")
    src.add_argument("--clean", metavar="IN_PLY", help="clean, decimate and / or flip this mesh (a PLY write_ply wrote) instead of building one")
    ap.add_argument("--out", required=True, help="mesh file (.ply)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.clean is not None:
        s = settings_from_args(a, a.out)
        no_views = [step[0] for step in EDIT_STEPS if step[2] and s.pop(step[0], None) is not None]
        try:
            steps = edit_settings(s)
        except ValueError as e:
            ap.error("--clean: %s" % e)
        for key in no_views:
            ap.error("--%s needs the views of --mvs: --clean IN.ply has none (python -m deep3d_aerial_amd.%s takes a mesh and "
                     "an MVS folder)" % (key, key))
    else:
        check_args(ap, a)
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is built on the GPU (no CPU fallback)")
    if a.clean is not None:
        if steps["clean"] is None:   # with every clean step off the mesh that was read is still checked
            steps["clean"] = clean_settings(s) + (close_holes_setting(s),)
        v, f = read_ply(a.clean)
        v, f = _edit(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), None, steps)   # the steps that need no views
        write_ply(a.out, v, f)
        print("mesh %s: %d vertices, %d triangles cleaned from %s" % (a.out, v.shape[0], f.shape[0], a.clean))
        return a.out
    views = load_mvs_views(a.mvs)
    v, f = build_and_write(views, settings_from_args(a, a.out))
    print("mesh %s: %d vertices, %d triangles from %d views" % (a.out, v.shape[0], f.shape[0], len(views)))
    return a.out


if __name__ == "__main__":
    # python -m runs this file as __main__, a second copy of its classes: the stages that take the views (collapse, subdivide)
    # check them against the package's MeshView, so the tool runs the package's main
    from deep3d_aerial_amd.mesh import main as _main

    _main()
