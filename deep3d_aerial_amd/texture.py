"""Texturing the surface mesh from the views.

The reference runs OpenMVS's TextureMesh after ReconstructMesh and RefineMesh.  The rules below are this project's own and do
not claim to match OpenMVS: the rejection of photo-inconsistent views, the smoothing of the view choice and global and local seam
levelling (all four below) are off by default.

* Input.  vertices [n,3] fp32 and faces [m,3] int32 on the GPU (mesh.extract, mesh.clean, mesh.read_ply), every index in
  0 .. n - 1; views: ortho.OrthoView records (id, K, E, depth, image) with distinct ids.
* Face geometry.  Corners a, b, c in fp64; nrm = (b - a) x (c - a) and g = ((a + b) + c) / 3, in fp64 with no contraction, each
  sum left to right.  A face with nrm = 0 gets no view.
* Candidate.  ortho's projection (p = R X + t, q = K p, u = q0 / q2, v = q1 / q2).  A view is a candidate for a face when every
  corner has p2 > 0, q2 > 0, 0 <= u <= W-1 and 0 <= v <= H-1; nrm . (C - g) > 0 (C = ortho.camera_center: the face is
  front-facing); the depth D at g's pixel (floor(v + .5), floor(u + .5)) is finite and > 0; and p2(g) <= D (1 + depth_tolerance)
  (default 0.01, as in ortho).
* Choice.  A = 0.5 |(ub - ua)(vc - va) - (uc - ua)(vb - va)| in fp64, the projected area in pixels; s = 1 / A; the view is
  rejected when A = 0 or s is not finite.  key = (bits(fp32(s)) << 32) | id; the smallest key wins (the view that sees the face
  largest, ties to the lower id); the empty key is INT64_MAX.  A minimum does not depend on view order, batching or ranks.
* Charts.  Two faces are in one chart when they share an edge (an unordered vertex pair, as mesh_clean's edges: (a,b) (b,c)
  (c,a) with unequal ends) and have the same winning id.  A face with no winner is in no chart (chart -1).  A chart's label is
  its smallest face index; charts are numbered in increasing label order.
* Rect.  Each corner's (u, v) in the chart's view with the selection's arithmetic; over the chart's corners
  x0 = max(0, floor(min u) - pad), x1 = min(W-1, ceil(max u) + pad), y0, y1 alike, all inclusive.  pad >= 1 (default 2), so
  bilinear taps at any texcoord stay inside the rect.
* Packing (host, deterministic).  Pages are page_size wide (default 8192, at least every view's W and H).  Page 0 reserves a
  2 x 2 block of the empty colour at (0, 0): it opens page 0's first shelf.  Charts are sorted by (rect height desc, width desc,
  label asc) and shelf-packed left to right, top to bottom; a shelf is as tall as its first chart (page 0's first at least 2);
  a shelf that does not fit under the last one opens a new page.  A page is as tall as the bottom of its last shelf.
* Atlas.  Texel (ox + dx, oy + dy) of a chart's rect is the RGB of pixel (x0 + dx, y0 + dy) of the chart's view, copied; every
  other texel is empty_color (default (166, 166, 166), the reference's nColEmpty 0x00A6A6A6).
* Texcoords.  Per face corner s = (u - x0 + ox + 0.5) / page_width, t = 1 - (v - y0 + oy + 0.5) / page_height, in fp64 (sums
  left to right), rounded to fp32; texnumber is the page.  A face with no winner gets (1 / page_width, 1 - 1 / H0) at its three
  corners on page 0, the centre of the empty block (H0 the height of page 0).
* Files.  <stem>.ply, binary little-endian: one `comment TextureFile <stem>_<k>.png` per page, `element vertex` (float x, y,
  z), `element face` with `property list uchar int vertex_indices`, `property list uchar float texcoord` (6 values) and
  `property int texnumber` -- the layout MeshLab reads and OpenMVS writes.  Pages are RGB8 PNGs beside it.

Seam levelling (level=..., --level): one smooth additive colour correction per chart that makes charts of
different views agree along their common border.  It runs after the fill and the rank merge and before the empty colour.
* Node.  A distinct (chart, vertex) pair over the corners of faces that have a winner, numbered in increasing (chart, vertex)
  order.
* Sample.  f[node] (RGB): the bilinear tap of the filled atlas at x = (u - x0) + ox, y = ((v - y0) + oy) + page_row, u and v the
  texcoord pass's projection of the vertex in the chart's view; in fp64, per channel ((w00 c00 + w10 c10) + w01 c01) + w11 c11
  with w00 = (1 - tx)(1 - ty), w10 = tx (1 - ty), w01 = (1 - tx) ty, w11 = tx ty, rounded to fp32.  pad >= 1 keeps the four taps
  inside the rect; at a rect the image's border cut, a tap past the rect repeats the rect's last texel (its weight is 0).
* Seam pair.  A distinct (vertex, chart c1 < chart c2) such that the vertex is an end of a seam edge between c1 and c2.  A seam
  edge is an edge shared by exactly two faces (of all faces, mesh_clean's edges) that both have winners and lie in different
  charts: an edge of three or more faces, or next to a face with no winner, makes no seam.
* Smoothness edge.  A distinct (chart, unordered vertex pair) over the edges of the chart's faces.
* Energy.  g[node] (RGB, the channels independent) minimises the sum over seam pairs of ((f_i + g_i) - (f_j + g_j))^2 + smooth *
  the sum over smoothness edges of (g_a - g_b)^2 + anchor * the sum over nodes of g^2: (L + anchor I) g = b, L the graph
  Laplacian with weight 1 on seam pairs and smooth on smoothness edges, b_i = the sum over i's seam pairs of f_j - f_i (fp32, in
  increasing j).  anchor > 0 makes the system positive definite.  Defaults smooth = 0.1, anchor = 1e-3: settings, not
  measurements.
* Solve.  Conjugate gradients from g = 0 on fp32 vectors, dot products in fp64; a channel stops (and is frozen) once
  |r| <= level_tolerance |b| (default 1e-4), all stop after level_iterations (default 500).  A p is kept as A r + beta A p_old.
* Coverage.  A texel of a chart's rect is a candidate of a face of that chart when d2 <= 2, d2 the squared distance in fp64, in
  texel coordinates (X = (u - x0) + ox, Y = (v - y0) + oy), from its centre to the face's projected triangle, 0 inside or on it:
  exactly the texels a bilinear tap at a point of the triangle can read.  The texel takes the face with the smallest int64 key
  (bits(fp32(d2)) << 32) | face; a texel that is no face's candidate keeps its colour.
* Apply.  With w the barycentric weights of the closest point of the covering triangle (fp64, rounded to fp32) the correction is
  (w0 g0 + w1 g1) + w2 g2 in fp32 and each channel becomes clamp(rint(colour + correction), 0, 255); alpha is unchanged.
The dot products are folded from fixed slots in a fixed order, so two runs give the same bits; the levelled pages do not depend
on view order or batching.

Local seam levelling (local=..., --level_local): a correction per texel that takes each side of a seam to the
mean of the two sides on the seam and fades out over a band of `radius` texels inside the chart.  It runs after the fill, the
rank merge and the levelling above (when that is on) and before the empty colour; with it off nothing changes.  Everything after
the colour taps is integer, so the levelled pages are the same bits for every run, view order, batching, rank split and solve path.
* Unit.  Corrections are integers in units of 1/64 grey level.
* Seam edge.  The levelling's above: an edge shared by exactly two faces of all faces, both with winners, in different charts.
  Its record is (a, b, c1, c2) with a < b the ends by vertex index and c1 < c2 the charts, so nothing depends on the face order;
  the seam edges are listed in increasing (a, b).  They come from the same (edge, face) pairs in a stable sort by edge that the
  levelling's graph is built from (level_edge_pairs), sorted once when both levellings run.
* Samples.  For a seam edge and each of its two charts the ends' atlas coordinates are X = (u - x0) + ox and
  Y = ((v - y0) + oy) + page_row, u and v the texcoord pass's projection (fp64, no contraction).  L_c = max(|Xb - Xa|, |Yb - Ya|)
  in chart c and S = ceil(max(L_c1, L_c2)) + 1 (no square root): consecutive samples lie at most one texel apart in either axis,
  in both charts.  S = 1 exactly when the ends coincide in both charts; two distinct ends inside one texel give S = 2, two samples
  of the same texel.  Sample k = 0 .. S - 1 lies at t = k / (S - 1) (fp64; t = 0 when S = 1) and P = Pa + t (Pb - Pa) per chart,
  each coordinate as a + t (b - a).  The colour of a sample in a chart is the levelling's bilinear tap of the atlas at P, in fp64
  and not rounded.  Per channel e = floor(32 (colour_c2 - colour_c1) + 0.5): half the step, in units.  Chart c1's texel
  (floor(X + 0.5), floor(Y + 0.5)) gets the record +e, chart c2's texel gets -e.  Such a texel lies within d2 <= 0.5 of a face of
  its chart, so it is covered; it is kept inside the rect (which it never leaves for a vertex the view sees).  An edge with a
  chart whose view is missing or an end that does not project in front of the view has no samples.
* Records.  Sample j of all (seam edges in their order, then k) writes record 2 j for chart c1 and 2 j + 1 for chart c2; the
  records are put in a stable sort by texel (row * page_size + column).  Only the sums below depend on them, so the order within
  a texel never shows in a page.
* Seam texel.  A texel with at least one record.  D = (2 sum(e) + n) // (2 n) per channel (floor division; the sum of its n records
  in int64): their mean, rounded half up.  A sort and a fold over runs; no float atomics, and no integer ones either.
* Domain and band.  A chart's domain is the texels of its rect that the coverage gives a face (d2 <= 2).  dist is the breadth-first
  distance over 4-neighbours inside the rect and the domain from the seam texels (dist 0), found in `radius` rounds; a texel is
  active when 1 <= dist <= radius.  A domain texel further away or not reachable keeps dist 255 and c = 0; a neighbour outside
  the rect or the domain is left out everywhere.  Rects of different charts touch in the atlas: a chart never reads another's texels.
* Solve.  c = D on seam texels and 0 elsewhere at the start.  A sweep updates the active texels with (X + Y) even, then those with
  (X + Y) odd, in place (X the atlas column, Y the atlas row, page_row included): c = (2 s + n) // (2 n) per channel, s the sum over
  the texel's in-domain 4-neighbours (active or not) and n their count; an active texel has n >= 1.  Texels of one parity are never
  neighbours, so a half-sweep has no order dependence.  |c| never exceeds the largest |D| (8160), so int16 holds it.  The solve
  stops after `iterations` sweeps or after the first sweep that changes nothing; sweeps past a fixed point change nothing, so the
  early stop never shows in the result, nor does the cadence (16 sweeps) at which the host looks at the counts.
* State.  One int64 per texel of the atlas, as the coverage: c of R, G, B as int16 in bits 0 .. 15, 16 .. 31, 32 .. 47; dist in bits
  48 .. 55; bit 56 "in the domain"; bit 57 "seam texel" (local_fields takes it apart).
* Paths.  A chart whose rect has at most lds_texels texels (default: 160 KiB / 8 bytes = 20480, a capacity and no tuning result)
  and whose padded image with its flags, (h + 2) (w + 1) + 4 words, fits into the 160 KiB is solved by one workgroup in LDS, band
  and sweeps; the launches are three, by the LDS a chart needs (16, 64 and 160 KiB per workgroup), so that small charts share a
  CU.  Every other chart runs as (chart, band of 8 rows) work items, one launch per dilation round and per half-sweep.  Both give
  the same bits.  "sweeps" is the number of sweeps that changed something, the largest over the charts, on either path;
  "converged" says that a sweep that changed nothing was reached: sweeps < iterations.
* Apply.  Every domain texel with dist <= radius gets channel = clamp(channel + ((c + 32) >> 6), 0, 255); alpha is unchanged.
* Settings.  radius 1 .. 254, default 16; iterations 1 .. 65535, default 512: settings, not measurements.  On a straight seam
  with radius 16 the iteration reaches a true fixed point in 161 .. 267 sweeps for |D| of 20 .. 127.5 levels, at most 0.5625 levels
  from the ramp D (1 - dist / 17) and exactly 0 past the radius (tests/test_texture_local.py).

Smoothing the view choice (smooth_views=..., --smooth_views W): each face may give up a bounded share of its
best projected area to agree with the faces around it, so that charts are fewer and larger.  It replaces the Choice above;
with it off nothing changes.
* Candidates.  cand [m, K] int64, K = 16 (d3d_texture_candidates_max): per face the K smallest of the keys that the Candidate
  and Choice tests accept over all views, in increasing order, padded with INT64_MAX.  Keys are distinct (the id is the low
  word), so the K smallest of a union do not depend on view order, batching or ranks; cand[:, 0] is the Choice's key.
* Winner.  A face has a winner when its three indices are distinct and cand[f, 0] is a key.  View ids are 0 .. 2^31 - 2.
* Data term.  s_k = the fp32 whose bits are cand[f, k] >> 32; d_k = 1 - s_0 / s_k in fp32 (an IEEE-rounded division, no
  contraction), in [0, 1): the share of its best projected area the face gives up.  Candidate k is admissible when it is a key
  and d_k <= max_loss; candidate 0 always is.
* Neighbours.  Two faces that both have a winner are neighbours when they share at least one vertex; the weight w_fg is the
  number of vertices they share (walking the three corner rows of f in the vertex -> face lists, skipping f itself, visits g
  exactly w_fg times).  Faces without a winner are walked over and not counted.
* Energy.  E = sum_f d(f, l_f) + weight * sum_{f<g} w_fg [id(l_f) != id(l_g)], l_f the index of the face's candidate.
* Round, all in fp32, products and sums rounded separately.  Propose: from l_f = 0 before the first round, n_k = the weighted
  count of neighbours whose current id differs from candidate k's id (an integer: the visit order does not matter);
  c_k = d_k + weight * float(n_k); best = the admissible k with the smallest (c_k, k); gain = c_{l_f} - c_best; when gain > 0,
  prio[f] = (bits(gain) << 32) | (2^32 - 1 - f) and prop[f] = best, else prio[f] = 0.  Commit: f takes prop[f] iff prio[f] > 0
  and prio[f] > prio[g] for every neighbour g.  No two neighbours change in one round, so each commit lowers E by its gain,
  and the face with the largest gain always commits, so the rounds end.
* Stop.  After the first round with no commit, or after `rounds` rounds.  commits[r] counts round r's commits; the host reads
  the counts once per 8 rounds, and rounds past the fixed point change nothing, so the cadence never shows in the result.
* Output.  label [m] int32 (-1 without a winner) and key[f] = cand[f, label[f]] (INT64_MAX without a winner): a key of the
  Choice's format, so charts, rects, fill, texcoords and levelling run on it unchanged.
* Settings.  weight > 0 has no default (the command line's help names 0.1, the reference's fRatioDataSmoothness); max_loss in
  [0, 1], default 0.25; rounds in 1 .. 1024, default 64: settings, not measurements.
The smoothed keys are the same bits run to run and for any view order, batching or rank split.  Unlike the unsmoothed keys
they depend on the face numbering, through the tie-break of the priorities only.

Rejecting outlier views (outliers={"threshold": t}, --outlier_threshold t): a view that shows a face in a colour
far from what most of its candidate views show (a car that moved, a specular roof, a wall the depth test missed) is struck from
the face's candidate list before the Choice.  It is a filter between the Candidates above and the choice; with it off nothing
changes.
* Colour of a face in a candidate view.  The corners' (u, v) are the texcoord pass's projection (fp64, no contraction).  Four
  sample points in image space, each sum left to right in fp64: s0 = ((p0 + p1) + p2) / 3 and, for i = 0, 1, 2,
  s_{i+1} = ((4 p_i + p_j) + p_k) / 6 with j < k the other two corners.  Each sample is ortho's bilinear tap (ortho.py "Colour":
  x0 = floor(u), fx = u - x0, taps clamped to the image, the four weighted taps summed in ortho's order in fp64), not rounded.
  Per channel q = clamp(floor((((t0 + t1) + t2) + t3) + 0.5), 0, 1020): four times the mean, in quarter grey levels, 10 bits.
  The slot's word is col = 2^30 | qR << 20 | qG << 10 | qB (int32); the word 0 means "no colour".  A slot gets a colour when
  its key is a key, its id is among the offered views, the face's indices are in range and every corner projects in front of
  the view with finite (u, v); otherwise the slot is left as it was.  So batches accumulate into one col [m, 16] and ranks write
  disjoint slots: a colour does not depend on view order, batching or ranks.
* Vote, all integer.  A slot is valid when its key is a key and its col != 0; n is the number of valid slots.  Faces with n < 3
  are left alone.  Per channel med_c is the lower median: the value of rank (n - 1) >> 1 among the valid values in increasing
  order.  dev_k = max_c |q_kc - med_c|, T = floor(threshold * 1020), and slot k is an outlier when dev_k > T.  When every valid
  slot is an outlier (the three channel medians may belong to different views) the face keeps its whole list and is counted as
  kept_all.  Slots with a key but no colour are neither counted nor removed.
* Output.  cand_out [m, 16]: the surviving keys in their order, padded with INT64_MAX (it may alias cand); rejected [m] int32 has
  bit k set when original slot k was removed.  cand_out[:, 0] is the new Choice; with smooth_views the smoothing runs on cand_out,
  so its s_0 is the best inlier and charts_before counts cand_out[:, 0].
* Settings.  threshold in (0, 1] has no default (the command line's help names 0.06, the reference's fOutlierThreshold); 3 views,
  4 samples and the median are settings, not measurements.
* Limit.  The rule assumes comparable exposure between the views: a gain spread beyond the threshold rejects honest views.

Faces are never reordered or renumbered: a shuffled face list gives the same key per face (without smoothing).  Chart labels, and so the packing,
follow the face order.  The hot passes are HIP kernels (csrc/texture.hip): select, charts (hooking and pointer jumping over
(edge, face) pairs that torch.sort orders), rects, fill and texcoords; the smoothing's kernels are in csrc/texture_smooth.hip,
the levelling's in csrc/texture_level.hip, the local levelling's in csrc/texture_local.hip, the outlier rejection's in
csrc/texture_outliers.hip.  No float atomics; the integer atomics are min / max, the count of a smoothing round's commits, the
four counters of the outlier vote and the count of texels a global sweep of the local levelling changed.

    python -m deep3d_aerial_amd.texture --mesh IN.ply --mvs MVS_FOLDER --out OUT.ply [--image_root DIR]
        [--depth_tolerance 0.01] [--views_per_batch N] [--page_size 8192] [--pad 2] [--outlier_threshold T]
        [--smooth_views W [--smooth_max_loss 0.25] [--smooth_rounds 64]]
        [--level [--level_smooth 0.1] [--level_anchor 1e-3] [--level_tolerance 1e-4] [--level_iterations 500]]
        [--level_local [--level_local_radius 16] [--level_local_iterations 512]]
"""
import argparse
import ctypes
import os

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .ortho import (DEFAULT_TOLERANCE, EMPTY_KEY, OrthoView, _ViewRecord, _batches, _check_views, camera_center, check_tolerance,
                    check_views_per_batch)

DEFAULT_PAGE = 8192
DEFAULT_PAD = 2
EMPTY_COLOR = (166, 166, 166)
BAND = 8   # atlas rows per fill work item (csrc/texture_shared.h TX_BAND)
DEFAULT_LEVEL_SMOOTH = 0.1
DEFAULT_LEVEL_ANCHOR = 1e-3
DEFAULT_LEVEL_TOLERANCE = 1e-4
DEFAULT_LEVEL_ITERATIONS = 500
DEFAULT_LOCAL_RADIUS = 16   # settings, not measurements
DEFAULT_LOCAL_ITERATIONS = 512
MAX_LOCAL_RADIUS = 254
MAX_LOCAL_ITERATIONS = 65535
LOCAL_UNIT = 64   # a correction of the local levelling is an integer in units of 1 / 64 grey level
LOCAL_WORD_BYTES = 8   # of its state per texel (csrc/texture_local.hip)
LOCAL_LDS_CLASSES = (16 << 10, 64 << 10, 160 << 10)   # LDS bytes per workgroup of the three launches of the chart-in-LDS solve
LOCAL_FAR = 255   # the distance of a texel the band did not reach
CANDIDATES = 16   # keys per face of the candidate lists (csrc/texture_shared.h TX_CANDIDATES)
DEFAULT_SMOOTH_MAX_LOSS = 0.25   # settings, not measurements
DEFAULT_SMOOTH_ROUNDS = 64
MAX_SMOOTH_ROUNDS = 1024
QUARTER_LEVELS = 1020   # a colour channel of the outlier vote: four times 0 .. 255
_NONE = EMPTY_KEY


class Camera(_geom.IdCamera):
    """A view's camera alone: id, K [3,3], E = Tcw [4,4] and the image size.  The rects and texcoords need no more, so rank 0
    computes them for views whose maps it does not hold.  OrthoView has the same attributes."""

    def __init__(self, id, K, E, W, H):
        _geom.IdCamera.__init__(self, id, K, E)
        self.W, self.H = int(W), int(H)


def _record(v):
    return v.record() if isinstance(v, OrthoView) else v.fill(_ViewRecord())   # a camera alone: no maps


def _table(views, device):
    """The d3d_ortho_view_t records of `views` sorted by id, in device memory (the kernels look ids up by bisection)."""
    views = sorted(views, key=lambda v: v.id)
    ids = [v.id for v in views]
    if len(set(ids)) != len(ids):
        raise ValueError("view ids must be unique (got %s)" % ids)
    arr = (_ViewRecord * max(len(views), 1))(*[_record(v) for v in views])
    return _geom.records(arr, device), len(views)


def _mesh_arrays(vertices, faces):
    return _geom.mesh_arrays(vertices, faces, 3, "textured")


def _check_key(key, m, device):
    _geom.check_tensor(key, "key", torch.int64, (m,), device, "the mesh")


def check_page_size(page_size, views=()):
    P = int(page_size)
    if P != page_size or P < 2 or P >= 1 << 20:
        raise ValueError("page_size %r must be an integer in 2 .. 2^20 - 1" % (page_size,))
    for v in views:
        if v.W > P or v.H > P:
            raise ValueError("page_size %d is smaller than view %d's %d x %d image" % (P, v.id, v.W, v.H))
    return P


def check_pad(pad):
    if int(pad) != pad or not 1 <= int(pad) < 1 << 20:
        raise ValueError("pad %r must be an integer >= 1" % (pad,))
    return int(pad)


def check_empty_color(color):
    c = tuple(int(x) for x in color)
    if len(c) != 3 or not all(0 <= x <= 255 for x in c):
        raise ValueError("empty_color %r must be three integers in 0..255" % (color,))
    return c


# ----------------------------------------------------------------------------------------
# the passes
# ----------------------------------------------------------------------------------------
def select_faces(vertices, faces, views, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, key=None):
    """Min-merges the keys of `views` (OrthoView) into key [m] int64 (a new INT64_MAX vector when None) and returns it.  The
    result does not depend on the batching or the order of the views."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    tol = check_tolerance(depth_tolerance)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    if key is None:
        key = torch.full((m,), EMPTY_KEY, dtype=torch.int64, device=vertices.device)
    _check_key(key, m, vertices.device)
    lib = _lib.load()
    for batch in _batches(views, vpb):
        recs, nv = _table(batch, vertices.device)
        scratch, nbytes = _geom.scratch(lib.d3d_texture_scratch_bytes, m, nv, device=vertices.device)
        rc = lib.d3d_texture_select(_ptr(vertices), n, _ptr(faces), m, _ptr(recs), nv, tol, _ptr(scratch), nbytes, _ptr(key), _stream())
        _lib.check(rc, "d3d_texture_select")
    return key


def charts(faces, key, n_vertices=None):
    """(chart [m] int32 -- the chart number of each face, -1 without a winner --, labels [n_charts] int64 -- each chart's
    smallest face index, increasing).  n_vertices: any bound above the largest index (default: faces.max() + 1)."""
    if not (isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("faces must be [m,3] int32")
    if faces.device.type != "cuda":
        raise RuntimeError("faces are on %s (no CPU fallback)" % faces.device)
    faces = faces.contiguous()
    m = int(faces.shape[0])
    _check_key(key, m, faces.device)
    if 3 * m >= 1 << 31:
        raise ValueError("%d faces: 3 m < 2^31" % m)
    n = int(n_vertices) if n_vertices is not None else (int(faces.max()) + 1 if m else 1)
    dev = faces.device
    lib = _lib.load()
    edge = torch.empty((3 * m,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_texture_edges(_ptr(faces), m, n, _ptr(key), _ptr(edge), _stream()), "d3d_texture_edges")
    live = torch.nonzero(edge != _NONE).flatten()
    pair_face = torch.div(live, 3, rounding_mode="floor")
    pair_edge = edge[live]
    # order by (edge, winner id): a stable sort by id, then a stable sort by edge
    o1 = torch.argsort(key[pair_face] & 0xffffffff, stable=True)
    o2 = torch.argsort(pair_edge[o1], stable=True)
    perm = o1[o2]
    edge_sorted = pair_edge[perm].contiguous()
    face_sorted = pair_face[perm].to(torch.int32).contiguous()
    del edge, live, pair_face, pair_edge, o1, o2, perm
    scratch, nbytes = _geom.scratch(lib.d3d_texture_scratch_bytes, m, 0, device=dev)
    label = torch.empty((max(m, 1),), dtype=torch.int32, device=dev)
    chart = torch.empty((m,), dtype=torch.int32, device=dev)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    rounds = ctypes.c_int(0)
    rc = lib.d3d_texture_charts(_ptr(edge_sorted), _ptr(face_sorted), int(edge_sorted.shape[0]), _ptr(key), m, _ptr(scratch), nbytes,
                                _ptr(label), _ptr(chart), _ptr(flag), _ptr(total), ctypes.byref(rounds), _stream())
    _lib.check(rc, "d3d_texture_charts")
    labels = torch.nonzero((chart >= 0) & (label[:m] == torch.arange(m, dtype=torch.int32, device=dev))).flatten()
    if int(labels.shape[0]) != int(total.item()):
        raise RuntimeError("d3d_texture_charts: %d roots, %d charts" % (int(labels.shape[0]), int(total.item())))
    return chart, labels


def chart_views(key, labels):
    """The winning id of each chart [n_charts] int32 (the low 32 bits of its label face's key)."""
    return (key[labels] & 0xffffffff).to(torch.int32)


def chart_rects(vertices, faces, key, chart, n_charts, cameras, pad=DEFAULT_PAD):
    """rect [n_charts, 4] int32 (x0, y0, x1, y1), inclusive, of every chart in its view.  cameras: Camera or OrthoView records
    of every winning view (ids looked up)."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    pad = check_pad(pad)
    _check_key(key, m, vertices.device)
    recs, nc = _table(cameras, vertices.device)
    rect = torch.empty((max(int(n_charts), 1), 4), dtype=torch.int32, device=vertices.device)
    rc = _lib.load().d3d_texture_rects(_ptr(vertices), n, _ptr(faces), m, _ptr(key), _ptr(chart.contiguous()), int(n_charts), _ptr(recs),
                                       nc, pad, _ptr(rect), _stream())
    _lib.check(rc, "d3d_texture_rects")
    rect = rect[:int(n_charts)]
    if n_charts and int(rect[:, 0].max()) == 2 ** 31 - 1:
        raise ValueError("a chart's view is missing from the cameras")
    return rect


class Packing(object):
    """place [n_charts, 3] int64 (page, ox, oy) and the page heights; every page is page_size wide."""

    def __init__(self, place, heights, page_size):
        self.place = place
        self.heights = [int(h) for h in heights]
        self.page_size = int(page_size)
        self.page_row = np.concatenate([[0], np.cumsum(self.heights)]).astype(np.int64)

    @property
    def n_pages(self):
        return len(self.heights)


def pack(rects, page_size=DEFAULT_PAGE):
    """Shelf packing of the rects (see the module docstring) on the host.  rects: [n_charts, 4] (x0, y0, x1, y1) inclusive."""
    r = np.asarray(rects.cpu().numpy() if isinstance(rects, torch.Tensor) else rects, np.int64).reshape(-1, 4)
    P = check_page_size(page_size)
    w, h = r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1
    nc = r.shape[0]
    if nc and (w.min() < 1 or h.min() < 1 or w.max() > P or h.max() > P):
        raise ValueError("rects must be non-empty and at most page_size %d on a side" % P)
    place = np.zeros((nc, 3), np.int64)
    order = np.lexsort((np.arange(nc), -w, -h))
    ws, hs = w[order], h[order]
    cw = np.concatenate([[0], np.cumsum(ws)])
    heights, page, y, i, first = [], 0, 0, 0, True
    while i < nc:   # one iteration per shelf
        x0 = 2 if first else 0
        j = int(np.searchsorted(cw, cw[i] + (P - x0), side="right")) - 1   # charts i .. j-1 fit: cw[j] - cw[i] <= P - x0
        if j == i:   # only on page 0's first shelf: the block alone
            y, first = 2, False
            continue
        sh = max(int(hs[i]), 2) if first else int(hs[i])
        if y + sh > P:
            heights.append(y)
            page, y = page + 1, 0
        place[order[i:j], 0] = page
        place[order[i:j], 1] = x0 + cw[i:j] - cw[i]
        place[order[i:j], 2] = y
        y += sh
        i, first = j, False
    heights.append(max(y, 2))
    return Packing(place, heights, P)


def chart_table(rects, packing, views_of_charts):
    """The kernels' chart table [n_charts, 8] int32: x0, y0, w, h, ox, oy, page, id (host array)."""
    r = np.asarray(rects.cpu().numpy() if isinstance(rects, torch.Tensor) else rects, np.int64).reshape(-1, 4)
    ids = np.asarray(views_of_charts.cpu().numpy() if isinstance(views_of_charts, torch.Tensor) else views_of_charts, np.int64)
    t = np.stack([r[:, 0], r[:, 1], r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1, packing.place[:, 1], packing.place[:, 2],
                  packing.place[:, 0], ids], 1) if r.shape[0] else np.zeros((0, 8), np.int64)
    return np.ascontiguousarray(t, np.int32)


def new_atlas(packing, device):
    """All pages as one zeroed int32 buffer [sum of heights, page_size] (packed RGBA8 texels)."""
    return torch.zeros((int(packing.page_row[-1]), packing.page_size), dtype=torch.int32, device=device)


def fill_pages(table, packing, views, atlas=None):
    """Copies the rects of the charts whose view is among `views` (OrthoView) into atlas (new_atlas when None); other texels are
    left as they are.  table: chart_table.  Returns the atlas."""
    views = _check_views(views)
    dev = views[0].depth.device if views else (atlas.device if atlas is not None else torch.device("cuda"))
    if atlas is None:
        atlas = new_atlas(packing, dev)
    if tuple(atlas.shape) != (int(packing.page_row[-1]), packing.page_size) or atlas.dtype != torch.int32 or not atlas.is_contiguous():
        raise ValueError("atlas must be a contiguous int32 tensor of shape (%d, %d)" % (int(packing.page_row[-1]), packing.page_size))
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    held = np.isin(table[:, 7], [v.id for v in views])
    nb = np.where(held, (table[:, 3].astype(np.int64) + BAND - 1) // BAND, 0)
    work = np.stack([np.repeat(np.arange(table.shape[0]), nb), np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)], 1)
    if not work.shape[0] or not views:
        return atlas
    check_page_size(packing.page_size, views)
    recs, nv = _table(views, atlas.device)
    w = torch.from_numpy(np.ascontiguousarray(work, np.int32)).to(atlas.device)
    t = torch.from_numpy(table).to(atlas.device)
    pr = torch.from_numpy(packing.page_row).to(atlas.device)
    rc = _lib.load().d3d_texture_fill(_ptr(w), int(w.shape[0]), _ptr(t), int(t.shape[0]), _ptr(pr), packing.n_pages, _ptr(recs), nv,
                                      packing.page_size, _ptr(atlas), _stream())
    _lib.check(rc, "d3d_texture_fill")
    return atlas


def finish_pages(atlas, empty_color=EMPTY_COLOR):
    """Every texel no fill wrote becomes the empty colour (alpha 255); in place.  Returns atlas."""
    c = check_empty_color(empty_color)
    rc = _lib.load().d3d_texture_empty(_ptr(atlas), int(atlas.numel()), c[0] | c[1] << 8 | c[2] << 16, _stream())
    _lib.check(rc, "d3d_texture_empty")
    return atlas


def split_pages(atlas, packing):
    """The pages as host RGB8 arrays [[H_k, page_size, 3] uint8]."""
    rgb = atlas.contiguous().view(torch.uint8).reshape(atlas.shape[0], atlas.shape[1], 4)[:, :, :3].cpu().numpy()
    return [np.ascontiguousarray(rgb[packing.page_row[k]:packing.page_row[k + 1]]) for k in range(packing.n_pages)]


# ----------------------------------------------------------------------------------------
# seam levelling
# ----------------------------------------------------------------------------------------
def check_level_settings(level):
    """The level settings dict checked: (smooth, anchor, tolerance, iterations)."""
    smooth = float(level.get("smooth", DEFAULT_LEVEL_SMOOTH))
    anchor = float(level.get("anchor", DEFAULT_LEVEL_ANCHOR))
    tol = float(level.get("tolerance", DEFAULT_LEVEL_TOLERANCE))
    it = level.get("iterations", DEFAULT_LEVEL_ITERATIONS)
    if not (np.isfinite(smooth) and smooth >= 0):
        raise ValueError("level_smooth %r must be finite and >= 0" % (smooth,))
    if not (np.isfinite(anchor) and anchor > 0):
        raise ValueError("level_anchor %r must be finite and > 0" % (anchor,))
    if not 0 < tol < 1:
        raise ValueError("level_tolerance %r must lie in (0, 1)" % (tol,))
    if int(it) != it or int(it) < 1:
        raise ValueError("level_iterations %r must be an integer >= 1" % (it,))
    return smooth, anchor, tol, int(it)


class LevelGraph(object):
    """nodes [N] int64 (chart * n_vertices + vertex, increasing), face_nodes [m, 3] int32 (-1: no chart), seams [S] and smooth
    [E] int64 ((i << 32) | j, i < j, distinct and increasing), and the CSR of the undirected weighted graph: row_ptr [N + 1],
    column [nnz] int32 (increasing within a row), weight [nnz] fp32.  All on the GPU."""

    def __init__(self, n_vertices, nodes, face_nodes, seams, smooth, row_ptr, column, weight):
        self.n_vertices = int(n_vertices)
        self.nodes, self.face_nodes, self.seams, self.smooth = nodes, face_nodes, seams, smooth
        self.row_ptr, self.column, self.weight = row_ptr, column, weight

    @property
    def n_nodes(self):
        return int(self.nodes.shape[0])


def _live(keys):
    return keys[keys != _NONE]


def _faces_and_chart(faces, chart, n_vertices):
    """(faces, chart, m, n, device) checked for the passes over the (edge, face) pairs."""
    if not (isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("faces must be [m,3] int32")
    if faces.device.type != "cuda":
        raise RuntimeError("faces are on %s (no CPU fallback)" % faces.device)
    faces = faces.contiguous()
    m, n, dev = int(faces.shape[0]), max(int(n_vertices), 1), faces.device
    if not (isinstance(chart, torch.Tensor) and chart.dtype == torch.int32 and tuple(chart.shape) == (m,) and chart.device == dev):
        raise ValueError("chart must be an int32 tensor of shape (%d,) on %s" % (m, dev))
    if 3 * m >= 1 << 31:
        raise ValueError("%d faces: 3 m < 2^31" % m)
    return faces, chart.contiguous(), m, n, dev


def level_edge_pairs(faces, chart, n_vertices):
    """What both levellings start from: (incidence [3 m] int64 -- the node key of every corner, INT64_MAX without a chart --,
    edge_sorted [n_pairs] int64, face_sorted [n_pairs] int32 -- the (edge, face) pairs of EVERY face in a stable sort by edge)."""
    faces, chart, m, n, dev = _faces_and_chart(faces, chart, n_vertices)
    inc = torch.empty((3 * m,), dtype=torch.int64, device=dev)
    edge = torch.empty((3 * m,), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().d3d_texture_level_incidence(_ptr(faces), m, n, _ptr(chart), _ptr(inc), _ptr(edge), _stream()),
               "d3d_texture_level_incidence")
    live = torch.nonzero(edge != _NONE).flatten()
    order = torch.argsort(edge[live], stable=True)
    edge_sorted = edge[live][order].contiguous()
    face_sorted = torch.div(live[order], 3, rounding_mode="floor").to(torch.int32).contiguous()
    return inc, edge_sorted, face_sorted


def level_graph(faces, chart, n_vertices, smooth=DEFAULT_LEVEL_SMOOTH, pairs=None):
    """The nodes, seam pairs, smoothness edges and CSR (LevelGraph) of the charts of `faces`.  pairs: level_edge_pairs' result for
    the same faces and charts, when the caller has it."""
    faces, chart, m, n, dev = _faces_and_chart(faces, chart, n_vertices)
    lib = _lib.load()
    inc, edge_sorted, face_sorted = pairs if pairs is not None else level_edge_pairs(faces, chart, n)
    nodes = torch.unique(_live(inc))
    n_pairs, N = int(edge_sorted.shape[0]), int(nodes.shape[0])
    del inc
    face_nodes = torch.empty((m, 3), dtype=torch.int32, device=dev)
    seam = torch.empty((2 * n_pairs,), dtype=torch.int64, device=dev)
    smooth_keys = torch.empty((3 * m,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_texture_level_pairs(_ptr(faces), m, n, _ptr(chart), _ptr(nodes), N, _ptr(edge_sorted), _ptr(face_sorted), n_pairs,
                                           _ptr(face_nodes), _ptr(seam), _ptr(smooth_keys), _stream()), "d3d_texture_level_pairs")
    seams, smooths = torch.unique(_live(seam)), torch.unique(_live(smooth_keys))
    both = torch.cat([seams, smooths])
    swapped = ((both & 0xffffffff) << 32) | (both >> 32)
    entry = torch.sort(torch.cat([both, swapped])).values.contiguous()
    nnz = int(entry.shape[0])
    if nnz >= 1 << 31:
        raise ValueError("%d graph entries: at most 2^31 - 1" % nnz)
    row_ptr = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    column = torch.empty((nnz,), dtype=torch.int32, device=dev)
    weight = torch.empty((nnz,), dtype=torch.float32, device=dev)
    _lib.check(lib.d3d_texture_level_csr(_ptr(entry), nnz, _ptr(nodes), N, n, float(smooth), _ptr(row_ptr), _ptr(column), _ptr(weight),
                                         _stream()), "d3d_texture_level_csr")
    return LevelGraph(n, nodes, face_nodes, seams, smooths, row_ptr, column, weight)


def _check_chart(chart, m, device):
    """The faces' chart numbers checked, contiguous."""
    if not (isinstance(chart, torch.Tensor) and chart.dtype == torch.int32 and tuple(chart.shape) == (m,)):
        raise ValueError("chart must be an int32 tensor of shape (%d,)" % m)
    if chart.device != device:
        raise RuntimeError("chart is on %s, the mesh on %s (no CPU fallback)" % (chart.device, device))
    return chart.contiguous()


def _check_atlas(atlas, packing, device):
    if not isinstance(atlas, torch.Tensor):
        raise TypeError("atlas must be a tensor")
    if atlas.device.type != "cuda" or atlas.device != device:
        raise RuntimeError("atlas is on %s, the mesh on %s (no CPU fallback)" % (atlas.device, device))
    if tuple(atlas.shape) != (int(packing.page_row[-1]), packing.page_size) or atlas.dtype != torch.int32 or not atlas.is_contiguous():
        raise ValueError("atlas must be a contiguous int32 tensor of shape (%d, %d)" % (int(packing.page_row[-1]), packing.page_size))


def _level_tables(table, packing, cameras, device):
    """(table tensor, n_charts, page_row tensor, camera records, n_cams) for the levelling kernels."""
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    t = torch.from_numpy(table if table.shape[0] else np.zeros((1, 8), np.int32)).to(device)
    recs, nc = _table(cameras, device)
    return t, int(table.shape[0]), torch.from_numpy(packing.page_row).to(device), recs, nc


def level_samples(vertices, graph, table, packing, cameras, atlas):
    """(f [N, 4], b [N, 4]) fp32 (R, G, B, 0): the nodes' taps of the filled atlas and the right-hand side."""
    if not (isinstance(vertices, torch.Tensor) and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3):
        raise ValueError("vertices must be [n,3] float32")
    if vertices.device.type != "cuda":
        raise RuntimeError("vertices are on %s (no CPU fallback)" % vertices.device)
    vertices, dev = vertices.contiguous(), vertices.device
    _check_atlas(atlas, packing, dev)
    N = graph.n_nodes
    if N and int(vertices.shape[0]) < graph.n_vertices:
        raise ValueError("%d vertices, the graph was built for %d" % (int(vertices.shape[0]), graph.n_vertices))
    t, n_charts, pr, recs, nc = _level_tables(table, packing, cameras, dev)
    f = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    b = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    rc = _lib.load().d3d_texture_level_samples(_ptr(vertices), graph.n_vertices, _ptr(graph.nodes), N, _ptr(graph.row_ptr),
                                               _ptr(graph.column), int(graph.column.shape[0]), _ptr(t), n_charts, _ptr(pr), packing.n_pages,
                                               _ptr(recs), nc, packing.page_size, _ptr(atlas), _ptr(f), _ptr(b), _stream())
    _lib.check(rc, "d3d_texture_level_samples")
    return f, b


def level_solve(graph, b, anchor=DEFAULT_LEVEL_ANCHOR, tolerance=DEFAULT_LEVEL_TOLERANCE, iterations=DEFAULT_LEVEL_ITERATIONS):
    """(g [N, 4] fp32, iterations run, True when every channel met the tolerance): conjugate gradients for (L + anchor I) g = b."""
    N, dev = graph.n_nodes, graph.nodes.device
    if not (isinstance(b, torch.Tensor) and b.dtype == torch.float32 and tuple(b.shape) == (N, 4) and b.is_contiguous()):
        raise ValueError("b must be a contiguous float32 tensor of shape (%d, 4)" % N)
    if b.device != dev:
        raise RuntimeError("b is on %s, the graph on %s (no CPU fallback)" % (b.device, dev))
    _, anchor, tolerance, iterations = check_level_settings({"anchor": anchor, "tolerance": tolerance, "iterations": iterations})
    lib = _lib.load()
    scratch, nbytes = _geom.scratch(lib.d3d_texture_level_scratch_bytes, N, device=dev)
    g = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    it, ok = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.d3d_texture_level_solve(_ptr(graph.row_ptr), _ptr(graph.column), _ptr(graph.weight), int(graph.column.shape[0]), _ptr(b), N,
                                     anchor, tolerance, iterations, _ptr(scratch), nbytes, _ptr(g), ctypes.byref(it), ctypes.byref(ok),
                                     _stream())
    _lib.check(rc, "d3d_texture_level_solve")
    return g, it.value, bool(ok.value)


def level_coverage(vertices, faces, chart, table, packing, cameras):
    """cover [atlas rows, page_size] int64: per texel the smallest (bits(fp32(d2)) << 32) | face, INT64_MAX where no face covers."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    dev = vertices.device
    chart = _check_chart(chart, m, dev)
    t, n_charts, pr, recs, nc = _level_tables(table, packing, cameras, dev)
    cover = torch.full((int(packing.page_row[-1]), packing.page_size), EMPTY_KEY, dtype=torch.int64, device=dev)
    rc = _lib.load().d3d_texture_level_cover(_ptr(vertices), n, _ptr(faces), m, _ptr(chart), _ptr(t), n_charts, _ptr(pr),
                                             packing.n_pages, _ptr(recs), nc, packing.page_size, _ptr(cover), _stream())
    _lib.check(rc, "d3d_texture_level_cover")
    return cover


def level_apply(vertices, faces, chart, graph, g, cover, table, packing, cameras, atlas):
    """Adds the correction to every covered texel of atlas, in place.  Returns atlas."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    dev = vertices.device
    chart = _check_chart(chart, m, dev)
    _check_atlas(atlas, packing, dev)
    N = graph.n_nodes
    if not (isinstance(g, torch.Tensor) and g.dtype == torch.float32 and tuple(g.shape) == (N, 4) and g.is_contiguous() and g.device == dev):
        raise ValueError("g must be a contiguous float32 tensor of shape (%d, 4) on %s" % (N, dev))
    if not (isinstance(cover, torch.Tensor) and cover.dtype == torch.int64 and cover.shape == atlas.shape and cover.is_contiguous() and
            cover.device == dev):
        raise ValueError("cover must be a contiguous int64 tensor of the atlas's shape on %s" % dev)
    tb = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    nb = (tb[:, 3].astype(np.int64) + BAND - 1) // BAND
    work = np.stack([np.repeat(np.arange(tb.shape[0]), nb), np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)], 1)
    if not work.shape[0] or not N:
        return atlas
    t, n_charts, pr, recs, nc = _level_tables(table, packing, cameras, dev)
    w = torch.from_numpy(np.ascontiguousarray(work, np.int32)).to(dev)
    rc = _lib.load().d3d_texture_level_apply(_ptr(w), int(w.shape[0]), _ptr(vertices), n, _ptr(faces), m, _ptr(chart),
                                             _ptr(graph.face_nodes), _ptr(g), N, _ptr(t), n_charts, _ptr(pr), packing.n_pages, _ptr(recs),
                                             nc, packing.page_size, _ptr(cover), _ptr(atlas), _stream())
    _lib.check(rc, "d3d_texture_level_apply")
    return atlas


def level_pages(vertices, faces, key, chart, table, packing, cameras, atlas, smooth=DEFAULT_LEVEL_SMOOTH, anchor=DEFAULT_LEVEL_ANCHOR,
                tolerance=DEFAULT_LEVEL_TOLERANCE, iterations=DEFAULT_LEVEL_ITERATIONS, keep=None):
    """Levels the seams of the filled (and merged) atlas in place, before finish_pages.  cameras: every winning view.  Returns
    {"nodes", "seams", "iterations", "converged"}.  keep: None, or a dict that receives what the local levelling can reuse:
    "pairs" (level_edge_pairs) and, when it was computed, "cover" (level_coverage)."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    _check_key(key, m, vertices.device)
    _check_atlas(atlas, packing, vertices.device)
    smooth, anchor, tolerance, iterations = check_level_settings({"smooth": smooth, "anchor": anchor, "tolerance": tolerance,
                                                                  "iterations": iterations})
    pairs = level_edge_pairs(faces, chart, n)
    if keep is not None:
        keep["pairs"] = pairs
    graph = level_graph(faces, chart, n, smooth, pairs)
    info = {"nodes": graph.n_nodes, "seams": int(graph.seams.shape[0]), "iterations": 0, "converged": True}
    if not info["seams"]:   # b = 0: g = 0, every texel keeps its colour
        return info
    _, b = level_samples(vertices, graph, table, packing, cameras, atlas)
    g, info["iterations"], info["converged"] = level_solve(graph, b, anchor, tolerance, iterations)
    cover = level_coverage(vertices, faces, chart, table, packing, cameras)
    if keep is not None:
        keep["cover"] = cover
    level_apply(vertices, faces, chart, graph, g, cover, table, packing, cameras, atlas)
    return info


# ----------------------------------------------------------------------------------------
# local seam levelling
# ----------------------------------------------------------------------------------------
def check_local_settings(local):
    """The local settings dict checked: (radius, iterations)."""
    unknown = set(local) - {"radius", "iterations"}
    if unknown:
        raise ValueError("local: unknown settings %s" % sorted(unknown))
    radius = local.get("radius", DEFAULT_LOCAL_RADIUS)
    it = local.get("iterations", DEFAULT_LOCAL_ITERATIONS)
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_LOCAL_RADIUS:
        raise ValueError("level_local_radius %r must be an integer in 1 .. %d" % (radius, MAX_LOCAL_RADIUS))
    if isinstance(it, bool) or int(it) != it or not 1 <= int(it) <= MAX_LOCAL_ITERATIONS:
        raise ValueError("level_local_iterations %r must be an integer in 1 .. %d" % (it, MAX_LOCAL_ITERATIONS))
    return int(radius), int(it)


def local_seams(faces, chart, n_vertices, pairs=None):
    """seams [n_seams, 4] int32 (a, b, c1, c2): the seam edges in increasing (a, b) order, a < b the ends, c1 < c2 the charts.
    pairs: level_edge_pairs' result, when the caller has it."""
    faces, chart, m, n, dev = _faces_and_chart(faces, chart, n_vertices)
    _, edge_sorted, face_sorted = pairs if pairs is not None else level_edge_pairs(faces, chart, n)
    n_pairs = int(edge_sorted.shape[0])
    seam = torch.empty((n_pairs, 4), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().d3d_texture_local_seams(_ptr(edge_sorted), _ptr(face_sorted), n_pairs, _ptr(chart), m, n, _ptr(seam), _stream()),
               "d3d_texture_local_seams")
    return seam[seam[:, 0] >= 0].contiguous()


def _check_seams(seams, device):
    if not (isinstance(seams, torch.Tensor) and seams.dtype == torch.int32 and seams.dim() == 2 and seams.shape[1] == 4):
        raise ValueError("seams must be an int32 tensor of shape (n_seams, 4)")
    if seams.device != device:
        raise RuntimeError("seams are on %s, the mesh on %s (no CPU fallback)" % (seams.device, device))
    return seams.contiguous()


def local_samples(vertices, seams, table, packing, cameras, atlas):
    """(texel [R] int64, rec [R, 3] int32): the records of every sample of every seam edge, in a stable sort by texel (the index
    row * page_size + column in the atlas) of the order (seam edge, sample, chart c1 then c2)."""
    if not (isinstance(vertices, torch.Tensor) and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3):
        raise ValueError("vertices must be [n,3] float32")
    if vertices.device.type != "cuda":
        raise RuntimeError("vertices are on %s (no CPU fallback)" % vertices.device)
    vertices, dev = vertices.contiguous(), vertices.device
    _check_atlas(atlas, packing, dev)
    seams = _check_seams(seams, dev)
    ns, n = int(seams.shape[0]), int(vertices.shape[0])
    t, n_charts, pr, recs, nc = _level_tables(table, packing, cameras, dev)
    lib = _lib.load()
    count = torch.zeros((ns,), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_texture_local_count(_ptr(vertices), n, _ptr(seams), ns, _ptr(t), n_charts, _ptr(pr), packing.n_pages, _ptr(recs),
                                           nc, packing.page_size, _ptr(count), _stream()), "d3d_texture_local_count")
    scan = torch.zeros((ns + 1,), dtype=torch.int64, device=dev)
    scan[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    total = int(scan[-1])
    if 2 * total >= 1 << 31:
        raise ValueError("%d seam samples: at most 2^30 - 1" % total)
    texel = torch.empty((2 * total,), dtype=torch.int64, device=dev)
    rec = torch.empty((2 * total, 3), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_texture_local_samples(_ptr(vertices), n, _ptr(seams), ns, _ptr(scan), total, _ptr(t), n_charts, _ptr(pr),
                                             packing.n_pages, _ptr(recs), nc, packing.page_size, _ptr(atlas), _ptr(texel), _ptr(rec),
                                             _stream()), "d3d_texture_local_samples")
    texel, order = torch.sort(texel, stable=True)
    return texel.contiguous(), rec[order].contiguous()


def _check_cover(cover, packing, device, name="cover"):
    shape = (int(packing.page_row[-1]), packing.page_size)
    if not (isinstance(cover, torch.Tensor) and cover.dtype == torch.int64 and tuple(cover.shape) == shape and cover.is_contiguous()):
        raise ValueError("%s must be a contiguous int64 tensor of shape (%d, %d)" % ((name,) + shape))
    if cover.device.type != "cuda" or cover.device != device:
        raise RuntimeError("%s is on %s (no CPU fallback)" % (name, cover.device))


def local_fold(texel, rec, cover, packing):
    """state [atlas rows, page_size] int64 (module docstring "State"): the domain of `cover` and the seam texels with their D."""
    dev = cover.device if isinstance(cover, torch.Tensor) else None
    _check_cover(cover, packing, dev)
    R = int(texel.shape[0])
    if not (texel.dtype == torch.int64 and texel.is_contiguous() and rec.dtype == torch.int32 and tuple(rec.shape) == (R, 3) and
            rec.is_contiguous() and texel.device == dev and rec.device == dev):
        raise ValueError("texel [R] int64 and rec [R, 3] int32 must be contiguous and on %s" % dev)
    state = torch.empty_like(cover)
    _lib.check(_lib.load().d3d_texture_local_fold(_ptr(texel), _ptr(rec), R, _ptr(cover), int(cover.numel()), _ptr(state), _stream()),
               "d3d_texture_local_fold")
    return state


def local_fields(state):
    """The state's fields: (c [rows, P, 3] int16, dist [rows, P] uint8, domain [rows, P] bool, seam [rows, P] bool)."""
    c = torch.stack([((state >> s) & 0xffff).to(torch.int16) for s in (0, 16, 32)], -1)
    return c, ((state >> 48) & 255).to(torch.uint8), ((state >> 56) & 1).bool(), ((state >> 57) & 1).bool()


def local_lds_texels():
    """The default of lds_texels: the texels whose state fills the 160 KiB of LDS of a CU.  A capacity, not a tuning result."""
    return int(_lib.load().d3d_texture_local_lds_words())


def _local_split(table, lds_texels):
    """(charts of the LDS path, one int array per LDS class; work [n, 2] of the global path's (chart, band) items; every chart's
    work).  A chart takes the LDS path when its rect has at most lds_texels texels and its padded image with the flags, (h + 2) (w + 1) + 4
    words, fits into the LDS."""
    tb = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    w, h = tb[:, 2].astype(np.int64), tb[:, 3].astype(np.int64)
    need = ((h + 2) * (w + 1) + 4) * LOCAL_WORD_BYTES
    cap = local_lds_texels()
    limit = cap if lds_texels is None else int(lds_texels)
    if limit < 0:
        raise ValueError("lds_texels %r must be >= 0" % (lds_texels,))
    in_lds = (w * h <= limit) & (need <= cap * LOCAL_WORD_BYTES)
    classes, lo = [], 0
    for hi in LOCAL_LDS_CLASSES:
        classes.append(np.flatnonzero(in_lds & (need > lo) & (need <= hi)).astype(np.int32))
        lo = hi

    def work(mask):
        nb = np.where(mask, (h + BAND - 1) // BAND, 0)
        return np.ascontiguousarray(np.stack([np.repeat(np.arange(tb.shape[0]), nb),
                                              np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)], 1), np.int32)

    return classes, work(~in_lds), work(np.ones(tb.shape[0], bool))


def _local_tables(table, packing, device):
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    t = torch.from_numpy(table if table.shape[0] else np.zeros((1, 8), np.int32)).to(device)
    return t, int(table.shape[0]), torch.from_numpy(packing.page_row).to(device)


def _local_run(state, table, packing, radius, iterations, lds_texels):
    """The band (iterations = 0) or the band and the sweeps on both paths, in place: (sweeps, charts_lds, charts_global)."""
    _check_cover(state, packing, state.device if isinstance(state, torch.Tensor) else None, "state")
    dev = state.device
    lib = _lib.load()
    classes, work, _ = _local_split(table, lds_texels)
    t, n_charts, pr = _local_tables(table, packing, dev)
    sweeps = torch.zeros((max(n_charts, 1),), dtype=torch.int32, device=dev)
    for charts_of, lds_bytes in zip(classes, LOCAL_LDS_CLASSES):
        if len(charts_of):
            lst = torch.from_numpy(charts_of).to(dev)
            _lib.check(lib.d3d_texture_local_chart(_ptr(lst), len(charts_of), _ptr(t), n_charts, _ptr(pr), packing.n_pages,
                                                   packing.page_size, _ptr(state), radius, iterations, lds_bytes, _ptr(sweeps), _stream()),
                       "d3d_texture_local_chart")
    run = ctypes.c_int(0)
    if work.shape[0]:
        w = torch.from_numpy(work).to(dev)
        _lib.check(lib.d3d_texture_local_band(_ptr(w), int(w.shape[0]), _ptr(t), n_charts, _ptr(pr), packing.n_pages, packing.page_size,
                                              _ptr(state), radius, _stream()), "d3d_texture_local_band")
        if iterations:
            changed = torch.empty((iterations,), dtype=torch.int32, device=dev)
            _lib.check(lib.d3d_texture_local_sweeps(_ptr(w), int(w.shape[0]), _ptr(t), n_charts, _ptr(pr), packing.n_pages,
                                                    packing.page_size, _ptr(state), radius, iterations, _ptr(changed), ctypes.byref(run),
                                                    _stream()), "d3d_texture_local_sweeps")
    n_lds = int(sum(len(c) for c in classes))
    return max(int(sweeps.max()), run.value), n_lds, n_charts - n_lds


def local_band(state, table, packing, radius=DEFAULT_LOCAL_RADIUS, lds_texels=None):
    """The distances of the state, in place (the solve computes them itself; this is the band alone).  Returns state."""
    radius, _ = check_local_settings({"radius": radius})
    _local_run(state, table, packing, radius, 0, lds_texels)
    return state


def local_solve(state, table, packing, radius=DEFAULT_LOCAL_RADIUS, iterations=DEFAULT_LOCAL_ITERATIONS, lds_texels=None):
    """The band and the relaxation on local_fold's state, in place: (state, {"sweeps" -- those that changed something, the largest
    over the charts --, "converged" -- a sweep that changed nothing was reached --, "charts_lds", "charts_global"}).  lds_texels:
    charts with more texels than this take the global path (default: what fits into the LDS; 0: every chart)."""
    radius, iterations = check_local_settings({"radius": radius, "iterations": iterations})
    sweeps, n_lds, n_global = _local_run(state, table, packing, radius, iterations, lds_texels)
    return state, {"sweeps": sweeps, "converged": sweeps < iterations, "charts_lds": n_lds, "charts_global": n_global}


def local_apply(state, table, packing, atlas, radius=DEFAULT_LOCAL_RADIUS):
    """Adds the correction to every domain texel within `radius` of a seam, in place.  Returns atlas."""
    radius, _ = check_local_settings({"radius": radius})
    _check_cover(state, packing, state.device if isinstance(state, torch.Tensor) else None, "state")
    _check_atlas(atlas, packing, state.device)
    _, _, work = _local_split(table, None)
    if not work.shape[0]:
        return atlas
    t, n_charts, pr = _local_tables(table, packing, state.device)
    w = torch.from_numpy(work).to(state.device)
    _lib.check(_lib.load().d3d_texture_local_apply(_ptr(w), int(w.shape[0]), _ptr(t), n_charts, _ptr(pr), packing.n_pages,
                                                   packing.page_size, _ptr(state), radius, _ptr(atlas), _stream()),
               "d3d_texture_local_apply")
    return atlas


def local_pages(vertices, faces, key, chart, table, packing, cameras, atlas, radius=DEFAULT_LOCAL_RADIUS,
                iterations=DEFAULT_LOCAL_ITERATIONS, cover=None, pairs=None, lds_texels=None):
    """Levels the seams of the filled (and merged, and globally levelled) atlas locally, in place, before finish_pages.  cameras:
    every winning view.  cover: level_coverage's result when the global levelling computed it; pairs: level_edge_pairs' likewise.
    Returns {"seam_edges", "seam_texels", "active", "sweeps", "converged"}."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    _check_key(key, m, vertices.device)
    _check_atlas(atlas, packing, vertices.device)
    chart = _check_chart(chart, m, vertices.device)
    radius, iterations = check_local_settings({"radius": radius, "iterations": iterations})
    seams = local_seams(faces, chart, n, pairs)
    info = {"seam_edges": int(seams.shape[0]), "seam_texels": 0, "active": 0, "sweeps": 0, "converged": True}
    if not info["seam_edges"]:   # no record: c = 0 everywhere, every texel keeps its colour
        return info
    texel, rec = local_samples(vertices, seams, table, packing, cameras, atlas)
    if cover is None:
        cover = level_coverage(vertices, faces, chart, table, packing, cameras)
    state = local_fold(texel, rec, cover, packing)
    state, solved = local_solve(state, table, packing, radius, iterations, lds_texels)
    _, dist, domain, seam = local_fields(state)
    info.update({"seam_texels": int(seam.sum()), "active": int((domain & (dist >= 1) & (dist <= radius)).sum()),
                 "sweeps": solved["sweeps"], "converged": solved["converged"]})
    local_apply(state, table, packing, atlas, radius)
    return info


# ----------------------------------------------------------------------------------------
# smoothing the view choice
# ----------------------------------------------------------------------------------------
def check_smooth_settings(smooth):
    """The smooth_views settings dict checked: (weight, max_loss, rounds).  weight has no default."""
    if "weight" not in smooth:
        raise ValueError("smooth_views needs a weight (> 0)")
    weight = float(smooth["weight"])
    max_loss = float(smooth.get("max_loss", DEFAULT_SMOOTH_MAX_LOSS))
    rounds = smooth.get("rounds", DEFAULT_SMOOTH_ROUNDS)
    unknown = set(smooth) - {"weight", "max_loss", "rounds"}
    if unknown:
        raise ValueError("smooth_views: unknown settings %s" % sorted(unknown))
    if not (np.isfinite(weight) and np.float32(weight) > 0):
        raise ValueError("smooth_views weight %r must be finite and > 0" % (weight,))
    if not 0 <= max_loss <= 1:
        raise ValueError("smooth_max_loss %r must lie in [0, 1]" % (max_loss,))
    if int(rounds) != rounds or not 1 <= int(rounds) <= MAX_SMOOTH_ROUNDS:
        raise ValueError("smooth_rounds %r must be an integer in 1 .. %d" % (rounds, MAX_SMOOTH_ROUNDS))
    return weight, max_loss, int(rounds)


def _check_cand(cand, m, device, name="cand"):
    if not (isinstance(cand, torch.Tensor) and cand.dtype == torch.int64 and tuple(cand.shape) == (m, CANDIDATES) and cand.is_contiguous()):
        raise ValueError("%s must be a contiguous int64 tensor of shape (%d, %d)" % (name, m, CANDIDATES))
    if cand.device != device:
        raise RuntimeError("%s is on %s, the mesh on %s (no CPU fallback)" % (name, cand.device, device))


def face_candidates(vertices, faces, views, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, cand=None):
    """Merges the keys of `views` (OrthoView) into cand [m, 16] int64 (a new INT64_MAX list when None) and returns it: per face
    the 16 smallest keys that select_faces' tests accept, increasing, padded with INT64_MAX.  The result does not depend on the
    batching or the order of the views, and cand[:, 0] is select_faces' key."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    tol = check_tolerance(depth_tolerance)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    lib = _lib.load()
    if lib.d3d_texture_candidates_max() != CANDIDATES:
        raise RuntimeError("the library keeps %d candidates per face, texture.py %d" % (lib.d3d_texture_candidates_max(), CANDIDATES))
    if cand is None:
        cand = torch.full((m, CANDIDATES), EMPTY_KEY, dtype=torch.int64, device=vertices.device)
    _check_cand(cand, m, vertices.device)
    for batch in _batches(views, vpb):
        recs, nv = _table(batch, vertices.device)
        scratch, nbytes = _geom.scratch(lib.d3d_texture_scratch_bytes, m, nv, device=vertices.device)
        rc = lib.d3d_texture_candidates(_ptr(vertices), n, _ptr(faces), m, _ptr(recs), nv, tol, _ptr(scratch), nbytes, _ptr(cand), _stream())
        _lib.check(rc, "d3d_texture_candidates")
    return cand


def merge_candidates(a, b):
    """The 16 smallest distinct keys per face of the lists a and b [m, 16], written into a, which is returned."""
    if not isinstance(a, torch.Tensor) or a.dim() != 2:
        raise ValueError("candidate lists are [m, %d] int64 tensors" % CANDIDATES)
    if a.device.type != "cuda":
        raise RuntimeError("the candidates are on %s (no CPU fallback)" % a.device)
    m = int(a.shape[0])
    _check_cand(a, m, a.device, "a")
    _check_cand(b, m, a.device, "b")
    _lib.check(_lib.load().d3d_texture_candidates_merge(_ptr(a), _ptr(b), m, _ptr(a), _stream()), "d3d_texture_candidates_merge")
    return a


def smooth_views(faces, n_vertices, cand, weight, max_loss=DEFAULT_SMOOTH_MAX_LOSS, rounds=DEFAULT_SMOOTH_ROUNDS):
    """The smoothed choice (module docstring): (key [m] int64, label [m] int32, commits [rounds run] int32 -- each round's number
    of changes, cut at the first round without one).  faces [m, 3] int32 on the GPU, cand: face_candidates' list."""
    from .mesh import face_incidence

    if not (isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("faces must be [m,3] int32")
    if faces.device.type != "cuda":
        raise RuntimeError("faces are on %s (no CPU fallback)" % faces.device)
    weight, max_loss, rounds = check_smooth_settings({"weight": weight, "max_loss": max_loss, "rounds": rounds})
    faces = faces.contiguous()
    m, n, dev = int(faces.shape[0]), int(n_vertices), faces.device
    _check_cand(cand, m, dev)
    lib = _lib.load()
    scratch, nbytes = _geom.scratch(lib.d3d_texture_smooth_scratch_bytes, m, device=dev)
    if nbytes == 0 or n < 0 or n >= 1 << 31:
        raise ValueError("%d vertices, %d faces: the smoothing needs 6 m < 2^31 (the vertex -> face lists)" % (n, m))
    if m and (int(faces.min()) < 0 or int(faces.max()) >= n):
        raise ValueError("a face index is outside 0 .. %d" % (n - 1))
    foff, finc = face_incidence(faces, n)
    label = torch.empty((m,), dtype=torch.int32, device=dev)
    key = torch.empty((m,), dtype=torch.int64, device=dev)
    commits = torch.zeros((rounds,), dtype=torch.int32, device=dev)
    run = ctypes.c_int(0)
    rc = lib.d3d_texture_smooth(_ptr(cand), m, _ptr(faces), n, _ptr(foff), _ptr(finc), weight, max_loss, rounds, _ptr(scratch), nbytes,
                                _ptr(label), _ptr(key), _ptr(commits), ctypes.byref(run), _stream())
    _lib.check(rc, "d3d_texture_smooth")
    c = commits[:run.value]
    if run.value and int(c[-1]) == 0:
        c = c[:-1]
    return key, label, c


def smooth_losses(cand, label):
    """d [m] fp32 of the chosen candidates (NaN without a winner): 1 - s_0 / s_label."""
    has = label >= 0
    k = torch.gather(cand, 1, label.clamp(min=0).long()[:, None])[:, 0]
    s0 = (cand[:, 0] >> 32).to(torch.int32).view(torch.float32)
    sk = (k >> 32).to(torch.int32).view(torch.float32)
    return torch.where(has, 1.0 - s0 / sk, torch.full_like(s0, float("nan")))


# ----------------------------------------------------------------------------------------
# rejecting outlier views
# ----------------------------------------------------------------------------------------
def check_outlier_settings(outliers):
    """The outliers settings dict checked: the threshold, which has no default."""
    unknown = set(outliers) - {"threshold"}
    if unknown:
        raise ValueError("outliers: unknown settings %s" % sorted(unknown))
    if "threshold" not in outliers:
        raise ValueError("outliers needs a threshold (in (0, 1])")
    t = float(outliers["threshold"])
    if not (np.isfinite(t) and 0 < t <= 1):
        raise ValueError("outlier_threshold %r must lie in (0, 1]" % (outliers["threshold"],))
    return t


def _check_col(col, m, device):
    if not (isinstance(col, torch.Tensor) and col.dtype == torch.int32 and tuple(col.shape) == (m, CANDIDATES) and col.is_contiguous()):
        raise ValueError("col must be a contiguous int32 tensor of shape (%d, %d)" % (m, CANDIDATES))
    if col.device != device:
        raise RuntimeError("col is on %s, the candidates on %s (no CPU fallback)" % (col.device, device))


def face_colors(vertices, faces, cand, views, views_per_batch=None, col=None):
    """The colour words of `views` (OrthoView) written into col [m, 16] int32 (a new zero tensor when None), which is returned:
    col[f, k] is the colour of face f in the view of cand[f, k] when that view is among `views`; other slots are left as they
    are.  The result does not depend on the batching or the order of the views."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    _check_cand(cand, m, vertices.device)
    if col is None:
        col = torch.zeros((m, CANDIDATES), dtype=torch.int32, device=vertices.device)
    _check_col(col, m, vertices.device)
    lib = _lib.load()
    for batch in _batches(views, vpb):
        recs, nv = _table(batch, vertices.device)
        rc = lib.d3d_texture_face_colors(_ptr(vertices), n, _ptr(faces), m, _ptr(cand), _ptr(recs), nv, _ptr(col), _stream())
        _lib.check(rc, "d3d_texture_face_colors")
    return col


def reject_outliers(cand, col, threshold, out=None):
    """The vote (module docstring): (cand_out [m, 16] int64, rejected [m] int32, counts [4] int32 -- faces tested, faces whose
    column 0 changed, slots removed, kept_all faces).  out: where cand_out goes (a new tensor when None); it may be cand."""
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2:
        raise ValueError("candidate lists are [m, %d] int64 tensors" % CANDIDATES)
    if cand.device.type != "cuda":
        raise RuntimeError("the candidates are on %s (no CPU fallback)" % cand.device)
    m, dev = int(cand.shape[0]), cand.device
    _check_cand(cand, m, dev)
    _check_col(col, m, dev)
    T = int(np.floor(check_outlier_settings({"threshold": threshold}) * QUARTER_LEVELS))
    if out is None:
        out = torch.empty_like(cand)
    _check_cand(out, m, dev, "out")
    rejected = torch.zeros((m,), dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    rc = _lib.load().d3d_texture_outliers(_ptr(cand), _ptr(col), m, T, _ptr(out), _ptr(rejected), _ptr(counts), _stream())
    _lib.check(rc, "d3d_texture_outliers")
    return out, rejected, counts


def outlier_summary(counts, threshold, m):
    """texture_mesh's "outliers" entry: the threshold and T, the faces, those with three coloured views or more (tested), those
    whose first choice was struck (changed), the slots struck (removed) and the faces that kept a list with no inlier."""
    c = [int(x) for x in (counts.cpu().tolist() if isinstance(counts, torch.Tensor) else counts)]
    return {"threshold": float(threshold), "T": int(np.floor(float(threshold) * QUARTER_LEVELS)), "faces": int(m), "tested": c[0],
            "changed": c[1], "removed": c[2], "kept_all": c[3]}


def texcoords(vertices, faces, key, chart, table, packing, cameras):
    """(texcoord [m, 6] fp32, texnumber [m] int32) on the GPU."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    _check_key(key, m, vertices.device)
    dev = vertices.device
    recs, nc = _table(cameras, dev)
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 8)
    t = torch.from_numpy(table if table.shape[0] else np.zeros((1, 8), np.int32)).to(dev)
    pr = torch.from_numpy(packing.page_row).to(dev)
    tc = torch.empty((m, 6), dtype=torch.float32, device=dev)
    tn = torch.empty((m,), dtype=torch.int32, device=dev)
    rc = _lib.load().d3d_texture_texcoords(_ptr(vertices), n, _ptr(faces), m, _ptr(key), _ptr(chart.contiguous()), _ptr(t),
                                           int(table.shape[0]), _ptr(pr), packing.n_pages, _ptr(recs), nc, packing.page_size, _ptr(tc),
                                           _ptr(tn), _stream())
    _lib.check(rc, "d3d_texture_texcoords")
    return tc, tn


def layout(vertices, faces, key, cameras, page_size=DEFAULT_PAGE, pad=DEFAULT_PAD):
    """Charts, rects and packing of the selected keys: (chart, labels, rects, packing, table).  cameras: every winning view."""
    P = check_page_size(page_size, cameras)
    chart, labels = charts(faces, key, int(vertices.shape[0]))
    n_charts = int(labels.shape[0])
    rects = chart_rects(vertices, faces, key, chart, n_charts, cameras, pad)
    packing = pack(rects, P)
    table = chart_table(rects, packing, chart_views(key, labels))
    return chart, labels, rects, packing, table


_smooth_views = smooth_views   # texture_mesh's argument has the function's name


def smooth_summary(cand, label, commits, rounds, charts_before):
    """texture_mesh's "smooth" entry: the rounds that changed something, whether the fixed point was reached within `rounds`,
    the charts of the unsmoothed keys, the mean and the largest d of the chosen views and the share of faces whose list is full."""
    d = smooth_losses(cand, label)
    d = d[label >= 0]
    n = int(commits.shape[0])
    return {"rounds": n, "converged": n < rounds, "commits": [int(c) for c in commits.cpu().tolist()], "charts_before": int(charts_before),
            "mean_loss": float(d.double().mean()) if d.numel() else 0.0, "max_loss": float(d.max()) if d.numel() else 0.0,
            "full_lists": float((cand[:, -1] != EMPTY_KEY).double().mean()) if cand.shape[0] else 0.0}


def texture_mesh(vertices, faces, views, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, page_size=DEFAULT_PAGE,
                 pad=DEFAULT_PAD, empty_color=EMPTY_COLOR, level=None, smooth_views=None, outliers=None, local=None):
    """Every pass on one process: {"key", "chart", "labels", "rects", "packing", "table", "pages" (host RGB8 arrays),
    "texcoord", "texnumber"}.  level: None, or the seam levelling's settings {"smooth", "anchor", "tolerance", "iterations"}
    (check_level_settings; {} for the defaults); the result then has "level" (level_pages' dict).  smooth_views: None, or the
    settings of the view choice's smoothing {"weight", "max_loss", "rounds"} (check_smooth_settings; weight must be given): the
    candidates pass then replaces select_faces, "key" is the smoothed key, and the result has "label", "cand" and "smooth"
    (smooth_summary's dict).  outliers: None, or the settings of the rejection of outlier views {"threshold"}
    (check_outlier_settings): the candidate lists are then filtered (face_colors, reject_outliers) before the choice -- the
    smoothing when smooth_views is given, else column 0 --, and the result has "cand" (the filtered lists), "rejected" and
    "outliers" (outlier_summary's dict).  local: None, or the local seam levelling's settings {"radius", "iterations"}
    (check_local_settings; {} for the defaults): it runs after the global levelling when that is on, and the result then has
    "local" (local_pages' dict)."""
    views = _check_views(views)
    check_page_size(page_size, views)
    if level is not None:
        smooth, anchor, tolerance, iterations = check_level_settings(level)
    if local is not None:
        local_radius, local_iterations = check_local_settings(local)
    res = {}
    if outliers is not None:
        threshold = check_outlier_settings(outliers)
        if smooth_views is not None:
            weight, max_loss, rounds = check_smooth_settings(smooth_views)
        cand = face_candidates(vertices, faces, views, depth_tolerance, views_per_batch)
        col = face_colors(vertices, faces, cand, views, views_per_batch)
        cand, rejected, counts = reject_outliers(cand, col, threshold, out=cand)
        del col
        res.update({"cand": cand, "rejected": rejected, "outliers": outlier_summary(counts, threshold, cand.shape[0])})
        if smooth_views is not None:
            key, label, commits = _smooth_views(faces, int(vertices.shape[0]), cand, weight, max_loss, rounds)
            before = charts(faces, cand[:, 0].contiguous(), int(vertices.shape[0]))[1]
            res.update({"label": label, "smooth": smooth_summary(cand, label, commits, rounds, before.shape[0])})
        else:
            key = cand[:, 0].contiguous()
    elif smooth_views is not None:
        weight, max_loss, rounds = check_smooth_settings(smooth_views)
        cand = face_candidates(vertices, faces, views, depth_tolerance, views_per_batch)
        key, label, commits = _smooth_views(faces, int(vertices.shape[0]), cand, weight, max_loss, rounds)
        before = charts(faces, cand[:, 0].contiguous(), int(vertices.shape[0]))[1]
        res.update({"label": label, "cand": cand, "smooth": smooth_summary(cand, label, commits, rounds, before.shape[0])})
    else:
        key = select_faces(vertices, faces, views, depth_tolerance, views_per_batch)
    chart, labels, rects, packing, table = layout(vertices, faces, key, views, page_size, pad)
    atlas = fill_pages(table, packing, views, new_atlas(packing, vertices.device))
    keep = {}
    if level is not None:
        res["level"] = level_pages(vertices, faces, key, chart, table, packing, views, atlas, smooth, anchor, tolerance, iterations,
                                   keep=keep if local is not None else None)
    if local is not None:
        res["local"] = local_pages(vertices, faces, key, chart, table, packing, views, atlas, local_radius, local_iterations,
                                   cover=keep.get("cover"), pairs=keep.get("pairs"))
    del keep
    atlas = finish_pages(atlas, empty_color)
    tc, tn = texcoords(vertices, faces, key, chart, table, packing, views)
    res.update({"key": key, "chart": chart, "labels": labels, "rects": rects, "packing": packing, "table": table,
                "pages": split_pages(atlas, packing), "texcoord": tc, "texnumber": tn})
    return res


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("nt", "u1"), ("t", "<f4", (6,)), ("k", "<i4")])


def texture_names(path, n_pages):
    stem = os.path.basename(str(path))
    stem = stem[:-4] if stem.endswith(".ply") else stem
    return ["%s_%d.png" % (stem, k) for k in range(n_pages)]


def textured_ply_header(n_vertices, n_faces, texture_files):
    comments = "".join("comment TextureFile %s\n" % f for f in texture_files)
    return ("ply\nformat binary_little_endian 1.0\n%selement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\nproperty int texnumber\n"
            "end_header\n" % (comments, n_vertices, n_faces)).encode("ascii")


def write_textured_ply(path, vertices, faces, texcoord, texnumber, pages):
    """Writes <path> (.ply) and its pages <stem>_<k>.png beside it.  Tensors on any device, or arrays; pages: [H_k, W, 3]
    uint8 arrays.  Returns the paths written (PLY first)."""
    from PIL import Image

    if not str(path).endswith(".ply"):
        raise ValueError("the textured mesh path must end in .ply (got %s)" % path)
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    v = np.ascontiguousarray(host(vertices), "<f4").reshape(-1, 3)
    f = host(faces).reshape(-1, 3)
    rec = np.empty((f.shape[0],), FACE_DTYPE)
    rec["n"], rec["v"], rec["nt"] = 3, f, 6
    rec["t"] = host(texcoord).reshape(-1, 6)
    rec["k"] = host(texnumber).reshape(-1)
    names = texture_names(path, len(pages))
    folder = os.path.dirname(os.path.abspath(str(path)))
    os.makedirs(folder, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(textured_ply_header(v.shape[0], f.shape[0], names))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())
    out = [str(path)]
    for name, page in zip(names, pages):
        p = os.path.join(folder, name)
        Image.fromarray(np.ascontiguousarray(page, np.uint8), "RGB").save(p, format="PNG")
        out.append(p)
    return out


def read_textured_ply(path):
    """(vertices [n,3] fp32, faces [m,3] int32, texcoord [m,6] fp32, texnumber [m] int32, texture file names) of a file
    write_textured_ply wrote."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    lines = data[:end].decode("ascii").split("\n")
    counts, files = {}, []
    for ln in lines:
        w = ln.split()
        if len(w) == 3 and w[0] == "element":
            counts[w[1]] = int(w[2])
        if len(w) == 3 and w[:2] == ["comment", "TextureFile"]:
            files.append(w[2])
    nv, nf = counts.get("vertex"), counts.get("face")
    if nv is None or nf is None or data[:end + 11] != textured_ply_header(nv, nf, files):
        raise ValueError("%s: not a PLY file write_textured_ply wrote" % path)
    body = data[end + 11:]
    if len(body) != nv * 12 + nf * FACE_DTYPE.itemsize:
        raise ValueError("%s: %d bytes of data, %d expected" % (path, len(body), nv * 12 + nf * FACE_DTYPE.itemsize))
    v = np.frombuffer(body[:nv * 12], "<f4").reshape(nv, 3).astype(np.float32)
    rec = np.frombuffer(body[nv * 12:], FACE_DTYPE)
    if nf and not ((rec["n"] == 3).all() and (rec["nt"] == 6).all()):
        raise ValueError("%s: only triangles with 6 texcoords are read" % path)
    return (v, rec["v"].astype(np.int32).reshape(nf, 3), rec["t"].astype(np.float32).reshape(nf, 6), rec["k"].astype(np.int32),
            files)


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix=""):
    ap.add_argument("--%sdepth_tolerance" % prefix, type=float, default=DEFAULT_TOLERANCE,
                    help="a face is hidden from a view when its centroid's depth exceeds the view's depth map by more than this share")
    ap.add_argument("--%sviews_per_batch" % prefix, type=int, default=None, help="views per selection call (default: all)")
    ap.add_argument("--%spage_size" % prefix, type=int, default=DEFAULT_PAGE, help="texture page width (>= every image's width and height)")
    ap.add_argument("--%spad" % prefix, type=int, default=DEFAULT_PAD, help="pixels of margin around every chart's rect (>= 1)")
    ap.add_argument("--%soutlier_threshold" % prefix, type=float, default=None, metavar="T",
                    help="strike from a face's candidates the views whose colour of it is further than this from the median of "
                         "its views, as a share of the range (in (0, 1]; 0.06 is the reference's fOutlierThreshold)")
    ap.add_argument("--%ssmooth_views" % prefix, type=float, default=None, metavar="W",
                    help="smooth the view choice over the mesh with this weight (> 0; 0.1 is the reference's fRatioDataSmoothness): "
                         "fewer, larger charts")
    ap.add_argument("--%ssmooth_max_loss" % prefix, type=float, default=DEFAULT_SMOOTH_MAX_LOSS,
                    help="the largest share of its best projected area a face may give up (0 .. 1)")
    ap.add_argument("--%ssmooth_rounds" % prefix, type=int, default=DEFAULT_SMOOTH_ROUNDS, help="at most this many rounds (1 .. 1024)")
    ap.add_argument("--%slevel" % prefix, action="store_true",
                    help="level the colour seams between charts of different views (one smooth additive correction per chart)")
    ap.add_argument("--%slevel_smooth" % prefix, type=float, default=DEFAULT_LEVEL_SMOOTH,
                    help="weight of the correction's smoothness inside a chart (>= 0)")
    ap.add_argument("--%slevel_anchor" % prefix, type=float, default=DEFAULT_LEVEL_ANCHOR, help="weight that pulls the correction to 0 (> 0)")
    ap.add_argument("--%slevel_tolerance" % prefix, type=float, default=DEFAULT_LEVEL_TOLERANCE,
                    help="the solve stops at |r| <= this * |b| (in (0, 1))")
    ap.add_argument("--%slevel_iterations" % prefix, type=int, default=DEFAULT_LEVEL_ITERATIONS, help="at most this many iterations (>= 1)")
    ap.add_argument("--%slevel_local" % prefix, action="store_true",
                    help="level the seams locally: a correction that fades out over a band of texels on both sides of every seam "
                         "(after --%slevel when both are given)" % prefix)
    ap.add_argument("--%slevel_local_radius" % prefix, type=int, default=DEFAULT_LOCAL_RADIUS,
                    help="the band's width in texels on each side of a seam (1 .. 254)")
    ap.add_argument("--%slevel_local_iterations" % prefix, type=int, default=DEFAULT_LOCAL_ITERATIONS,
                    help="at most this many sweeps of the relaxation (1 .. 65535)")


def check_settings(settings):
    """The settings dict checked: (depth_tolerance, views_per_batch, page_size, pad)."""
    return (check_tolerance(settings.get("depth_tolerance", DEFAULT_TOLERANCE)), check_views_per_batch(settings.get("views_per_batch")),
            check_page_size(settings.get("page_size", DEFAULT_PAGE)), check_pad(settings.get("pad", DEFAULT_PAD)))


def check_args(ap, a, prefix=""):
    """The argument errors of the texture settings, reported through ap.error."""
    try:
        check_settings(settings_from_args(a, None, prefix))
    except ValueError as e:
        ap.error("--%s*: %s" % (prefix, e))


def settings_from_args(a, path, prefix=""):
    g = lambda k: getattr(a, prefix + k)
    level = {"smooth": g("level_smooth"), "anchor": g("level_anchor"), "tolerance": g("level_tolerance"), "iterations": g("level_iterations")}
    check_level_settings(level)   # the numbers are checked whether or not --level is given
    local = {"radius": g("level_local_radius"), "iterations": g("level_local_iterations")}
    check_local_settings(local)   # likewise
    w = g("smooth_views")
    smooth = {"weight": 1.0 if w is None else w, "max_loss": g("smooth_max_loss"), "rounds": g("smooth_rounds")}
    check_smooth_settings(smooth)   # likewise
    t = g("outlier_threshold")
    outliers = None
    if t is not None:
        outliers = {"threshold": t}
        check_outlier_settings(outliers)
    s = {"path": path, "depth_tolerance": g("depth_tolerance"), "views_per_batch": g("views_per_batch"), "page_size": g("page_size"),
         "pad": g("pad"), "level": level if g("level") else None, "smooth_views": smooth if w is not None else None,
         "outliers": outliers, "local": local if g("level_local") else None}
    # the orthophoto of the textured mesh (ortho_mesh.py): only predict has the flags (--texture_ortho O.tif, --texture_ortho_*)
    if getattr(a, prefix + "ortho", None) is not None:
        from . import ortho_mesh as _ortho_mesh

        s["ortho"] = _ortho_mesh.settings_from_args(a, g("ortho"), prefix + "ortho_")
    return s


def build_and_write(vertices, faces, views, settings):
    """texture_mesh with the settings dict, written to settings["path"]: the result dict."""
    tol, vpb, P, pad = check_settings(settings)
    res = texture_mesh(vertices, faces, views, tol, vpb, P, pad, level=settings.get("level"), smooth_views=settings.get("smooth_views"),
                       outliers=settings.get("outliers"), local=settings.get("local"))
    write_textured_ply(settings["path"], vertices, faces, res["texcoord"], res["texnumber"], res["pages"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description="texture a surface mesh (binary PLY) from predict's depth maps, cameras and images")
    ap.add_argument("--mesh", required=True, help="the mesh (a PLY mesh.write_ply wrote)")
    ap.add_argument("--mvs", required=True, help="predict's output folder: {name}_init.pfm and {name}.txt")
    ap.add_argument("--out", required=True, help="textured mesh file (.ply; the <stem>_<k>.png pages are written beside it)")
    ap.add_argument("--image_root", default=None, help="folder the camera files' relative image paths start from")
    add_arguments(ap)
    a = ap.parse_args(argv)
    check_args(ap, a)
    if not a.out.endswith(".ply"):
        ap.error("--out must end in .ply")
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is textured on the GPU (no CPU fallback)")
    from .mesh import read_ply
    from .ortho import load_mvs_views

    v, f = read_ply(a.mesh)
    views = load_mvs_views(a.mvs, a.image_root)
    res = build_and_write(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), views, settings_from_args(a, a.out))
    print("textured mesh %s: %d faces, %d charts, %d pages, %d views" % (a.out, f.shape[0], int(res["labels"].shape[0]),
                                                                        res["packing"].n_pages, len(views)))
    if "outliers" in res:
        o = res["outliers"]
        print("rejected outlier views: threshold %g (T = %d), %d of %d faces tested, %d slots removed, %d faces changed their first view, "
              "%d kept a list without an inlier" % (o["threshold"], o["T"], o["tested"], o["faces"], o["removed"], o["changed"], o["kept_all"]))
    if "smooth" in res:
        print("smoothed the view choice in %d rounds%s: %d charts before, mean loss %.4f, largest %.4f" %
              (res["smooth"]["rounds"], "" if res["smooth"]["converged"] else " (not converged)", res["smooth"]["charts_before"],
               res["smooth"]["mean_loss"], res["smooth"]["max_loss"]))
    if "level" in res:
        print("levelled %d seam pairs over %d nodes in %d iterations%s" % (res["level"]["seams"], res["level"]["nodes"], res["level"]["iterations"],
                                                                          "" if res["level"]["converged"] else " (not converged)"))
    if "local" in res:
        print("levelled locally: %d seam edges, %d seam texels, %d texels in the band, %d sweeps%s" %
              (res["local"]["seam_edges"], res["local"]["seam_texels"], res["local"]["active"], res["local"]["sweeps"],
               "" if res["local"]["converged"] else " (not converged)"))
    return a.out


if __name__ == "__main__":
    main()
