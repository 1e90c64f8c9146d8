"""Refining the surface mesh against the images on the GPU (csrc/mesh_refine.hip): the step the reference
runs between ReconstructMesh and TextureMesh (mesh/createmesh.py:145-172, OpenMVS RefineMesh).  This stage does not claim to match
OpenMVS, which runs a gradient flow with subdivision: it is a plane sweep per vertex along the vertex normal, then a screened
smoothing of the scalar displacement.  Only vertices move: topology, face order and vertex count stay, so every later stage runs
on the result unchanged.  Off unless asked for.  The rule, in full (tests/test_mesh_refine.py restates it in numpy and the kernels
are held bit-equal to that):

Frames (per vertex).  N = the sum, over the faces of the vertex in the order of mesh.face_incidence's row, of (b - a) x (c - a) in
fp64 (a, b, c the face's corners in its own order); faces with an index out of range or repeated are skipped.  L =
sqrt((Nx^2 + Ny^2) + Nz^2), n = N / L.  A vertex is inactive, and never moves, when it has no such face, when N or L is not finite
or L = 0, or when mesh.adjacency marks it fixed (a boundary vertex).  Tangents: j = the axis of smallest |n_j| (ties to the lowest
j), c = e_j x n written out as (0, -nz, ny) | (nz, 0, -nx) | (-ny, nx, 0), t1 = c / sqrt((cx^2 + cy^2) + cz^2), t2 = n x t1.
Everything is fp64 without contraction, sums left to right.

Views of a vertex.  View V sees vertex X when p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1 (ortho's projection), dot =
(nx dx + ny dy) + nz dz > 0 with d = C - X, the depth D at pixel (floor(v + 0.5), floor(u + 0.5)) is finite and > 0, and
p2 <= D (1 + depth_tolerance) + reach * step.  s = 1 - dot / sqrt((dx^2 + dy^2) + dz^2); key = (bits(fp32(s)) << 32) | id.  The
vertex keeps its VIEWS = 4 smallest distinct keys, padded with INT64_MAX; the list is min-merged over calls, so it does not depend
on the order or the batching of the views.  A vertex with fewer than two keys does not move.

Hypotheses.  k = 0 .. 2 reach (reach 1 .. 7): X_k = X + ((k - reach) step) n.

Patch.  5 x 5 points (X_k + (a spacing) t1) + (b spacing) t2, a, b = -2 .. 2, b-major.  A point is valid in a view when p2 > 0,
q2 > 0, 0 <= u <= W-1 and 0 <= v <= H-1; its grey there is ortho's bilinear tap (fp64, unrounded) summed over the channels in
quarter levels: q = clamp(floor(4 ((tR + tG) + tB) + 0.5), 0, 3060), an integer.

Pair score.  Pairs are (slot 0, slot j), j = 1 .. 3, over the slots whose views are in the call's table with an image.  With
N = 25 and int64 sums over the patch: num = N S(ab) - S(a) S(b), va = N S(aa) - S(a)^2, vb alike.  A pair is valid at k when all
25 points are valid in both views and va, vb >= Tv = floor(625 * 144 * min_contrast^2) (the variance of the grey in levels^2,
scaled as the sums are; computed on the host, at least 1).  z = (double)num / sqrt((double)va (double)vb).  A pair is used only
when it is valid at every k; score_k = (the sum of z over the used pairs, in pair order) / their number.  With no used pair the
vertex does not move.

Pick.  k* = the k of largest score, ties to the smaller |k - reach|, then the smaller k.  w = 0 when score_k* < min_score, else 1.
When 0 < k* < 2 reach and den = (s- - 2 s0) + s+ < 0, delta = clamp(0.5 (s- - s+) / den, -0.5, 0.5), else 0.
d0 = fp32(((k* - reach) + delta) step).

Relax.  fp32, every operation rounded, neighbours in the order of mesh.adjacency's rows: d = w d0, then smooth_iterations Jacobi
steps d <- (w d0 + lambda m) / (w + lambda), m = (the sum of the neighbours' d) / float(degree).  Inactive vertices hold d = 0 and
count as neighbours.

Apply.  X <- fp32(X + (double)d n) per component, active vertices only.

Scales.  The whole sequence runs `scales` times; step and spacing are multiplied by scale_step after each (the reference's
--scales and fScaleStep).

The defaults below (reach 4, scales 2, scale_step 0.5, min_score 0.6, min_contrast 2 grey levels, smooth 1, smooth_iterations 10,
depth_tolerance 0.01) are settings, not measurements.  step has no default: it is a world length, half the mesh's voxel is a
start; spacing defaults to step.

Out of scope: subdivision and edge-size control, a gradient flow on the full photometric energy, image pyramids, moving boundary
vertices, matching sharded over ranks.

Command line:
    python -m deep3d_aerial_amd.refine --mesh IN.ply --mvs MVS --out OUT.ply --step S [--image_root DIR] [--reach 4] [--spacing S]
        [--scales 2] [--scale_step 0.5] [--min_score 0.6] [--min_contrast 2] [--smooth 1] [--smooth_iterations 10]
        [--depth_tolerance 0.01] [--views_per_batch N]
"""
import argparse
import math

import numpy as np
import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .ortho import DEFAULT_TOLERANCE, EMPTY_KEY, _batches, _check_views, check_tolerance, check_views_per_batch
from .texture import _table

VIEWS = 4   # keys per vertex of the view lists (csrc/mesh_refine.hip RF_VIEWS)
MAX_REACH = 7
MAX_SCALES = 8
# settings, not measurements
DEFAULT_REACH = 4
DEFAULT_SCALES = 2
DEFAULT_SCALE_STEP = 0.5
DEFAULT_MIN_SCORE = 0.6
DEFAULT_MIN_CONTRAST = 2.0
DEFAULT_SMOOTH = 1.0
DEFAULT_SMOOTH_ITERATIONS = 10
MAX_SMOOTH_ITERATIONS = 100000
_KEYS = ("step", "spacing", "reach", "scales", "scale_step", "min_score", "min_contrast", "smooth", "smooth_iterations", "depth_tolerance",
         "views_per_batch")


def min_variance(min_contrast):
    """Tv = floor(625 * 144 * min_contrast^2): the least 25^2 * variance of q = 12 * grey a patch needs in a view."""
    return int(math.floor(625.0 * 144.0 * (float(min_contrast) * float(min_contrast))))


def check_refine_settings(settings):
    """The settings dict checked and completed: {"step", "spacing", "reach", "scales", "scale_step", "min_score", "min_contrast",
    "smooth", "smooth_iterations", "depth_tolerance", "views_per_batch"}.  step has no default."""
    unknown = set(settings) - set(_KEYS)
    if unknown:
        raise ValueError("refine: unknown settings %s" % sorted(unknown))
    if settings.get("step") is None:
        raise ValueError("refine needs a step (a world length > 0; half the mesh's voxel is a start)")
    g = lambda k, d: d if settings.get(k) is None else settings[k]
    step = float(settings["step"])
    spacing = float(g("spacing", step))
    scale_step = float(g("scale_step", DEFAULT_SCALE_STEP))
    min_score = float(g("min_score", DEFAULT_MIN_SCORE))
    min_contrast = float(g("min_contrast", DEFAULT_MIN_CONTRAST))
    smooth = float(g("smooth", DEFAULT_SMOOTH))
    reach, scales, its = g("reach", DEFAULT_REACH), g("scales", DEFAULT_SCALES), g("smooth_iterations", DEFAULT_SMOOTH_ITERATIONS)
    for name, x in (("step", step), ("spacing", spacing), ("scale_step", scale_step), ("min_contrast", min_contrast), ("smooth", smooth)):
        if not (math.isfinite(x) and x > 0):
            raise ValueError("refine: %s %r must be finite and > 0" % (name, x))
    if scale_step > 1:
        raise ValueError("refine: scale_step %r must lie in (0, 1]" % scale_step)
    if not (math.isfinite(min_score) and -1 <= min_score <= 1):
        raise ValueError("refine: min_score %r must lie in -1 .. 1" % min_score)
    for name, x, lo, hi in (("reach", reach, 1, MAX_REACH), ("scales", scales, 1, MAX_SCALES),
                            ("smooth_iterations", its, 0, MAX_SMOOTH_ITERATIONS)):
        if isinstance(x, float) and not math.isfinite(x) or int(x) != x or not lo <= int(x) <= hi:
            raise ValueError("refine: %s %r must be an integer in %d .. %d" % (name, x, lo, hi))
    if not np.isfinite(np.float32(smooth)) or np.float32(smooth) <= 0:
        raise ValueError("refine: smooth %r must be a positive fp32 value" % smooth)
    if not (math.isfinite(min_contrast * min_contrast) and 1 <= min_variance(min_contrast) < 1 << 62):
        raise ValueError("refine: min_contrast %r is out of range (floor(90000 min_contrast^2) must be >= 1)" % min_contrast)
    last = step * scale_step ** (int(scales) - 1)
    if not (last > 0 and spacing * scale_step ** (int(scales) - 1) > 0):
        raise ValueError("refine: step %r and spacing %r vanish after %d scales of %r" % (step, spacing, scales, scale_step))
    return {"step": step, "spacing": spacing, "reach": int(reach), "scales": int(scales), "scale_step": scale_step, "min_score": min_score,
            "min_contrast": min_contrast, "smooth": smooth, "smooth_iterations": int(its),
            "depth_tolerance": check_tolerance(g("depth_tolerance", DEFAULT_TOLERANCE)),
            "views_per_batch": check_views_per_batch(settings.get("views_per_batch"))}


def _mesh_arrays(vertices, faces):
    vertices, faces, n, m = _geom.mesh_arrays(vertices, faces, 6, "refined")
    if n == 0:
        raise ValueError("the mesh has no vertex")
    return vertices, faces, n, m


def _check(t, name, dtype, shape, device):
    _geom.check_tensor(t, name, dtype, shape, device, "the mesh")


class Topology(object):
    """What the passes need of the faces, built once per mesh: the vertex -> face CSR and the neighbour CSR with its fixed flags."""

    def __init__(self, faces, n_vertices):
        from .mesh import adjacency, face_incidence

        self.face_offset, self.face_index = face_incidence(faces, n_vertices)
        self.offset, self.nbr, self.fixed = adjacency(faces, n_vertices)


# ----------------------------------------------------------------------------------------
# the passes
# ----------------------------------------------------------------------------------------
def vertex_frames(vertices, faces, topology=None):
    """(frame [n, 9] fp64 = (n, t1, t2) per vertex, active [n] uint8) on the GPU (module docstring, Frames)."""
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    topo = topology or Topology(faces, n)
    frame = torch.empty((n, 9), dtype=torch.float64, device=vertices.device)
    active = torch.empty((n,), dtype=torch.uint8, device=vertices.device)
    rc = _lib.load().d3d_mesh_refine_frames(_ptr(vertices), n, _ptr(faces), m, _ptr(topo.face_offset), _ptr(topo.face_index), _ptr(topo.fixed),
                                            _ptr(frame), _ptr(active), _stream())
    _lib.check(rc, "d3d_mesh_refine_frames")
    return frame, active


def vertex_views(vertices, frame, active, views, step, reach=DEFAULT_REACH, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, lists=None):
    """Merges the keys of `views` (OrthoView) into lists [n, 4] int64 (a new INT64_MAX list when None) and returns it (module
    docstring, Views of a vertex).  The result does not depend on the batching or the order of the views."""
    if not isinstance(vertices, torch.Tensor) or vertices.device.type != "cuda":
        raise RuntimeError("the mesh is refined on the GPU (no CPU fallback)")
    n, dev = int(vertices.shape[0]), vertices.device
    _check(vertices, "vertices", torch.float32, (n, 3), dev)
    _check(frame, "frame", torch.float64, (n, 9), dev)
    _check(active, "active", torch.uint8, (n,), dev)
    tol = check_tolerance(depth_tolerance)
    vpb = check_views_per_batch(views_per_batch)
    views = _check_views(views)
    lib = _lib.load()
    if lib.d3d_mesh_refine_views_max() != VIEWS:
        raise RuntimeError("the library keeps %d views per vertex, refine.py %d" % (lib.d3d_mesh_refine_views_max(), VIEWS))
    if lists is None:
        lists = torch.full((n, VIEWS), EMPTY_KEY, dtype=torch.int64, device=dev)
    _check(lists, "lists", torch.int64, (n, VIEWS), dev)
    for batch in _batches(views, vpb):
        recs, nv = _table(batch, dev)
        rc = lib.d3d_mesh_refine_views(_ptr(vertices), n, _ptr(frame), _ptr(active), _ptr(recs), nv, tol, int(reach), float(step), _ptr(lists),
                                       _stream())
        _lib.check(rc, "d3d_mesh_refine_views")
    return lists


def match(vertices, frame, active, lists, views, step, spacing=None, reach=DEFAULT_REACH, min_score=DEFAULT_MIN_SCORE,
          min_contrast=DEFAULT_MIN_CONTRAST):
    """The sweep and the pick over the views of `views` (OrthoView; a slot whose view is not among them is absent): (kstar [n] int32,
    weight [n] fp32, d0 [n] fp32, counts [4] int32 -- active vertices, vertices with two views or more, vertices with a used pair,
    vertices moved)."""
    if not isinstance(vertices, torch.Tensor) or vertices.device.type != "cuda":
        raise RuntimeError("the mesh is refined on the GPU (no CPU fallback)")
    n, dev = int(vertices.shape[0]), vertices.device
    _check(vertices, "vertices", torch.float32, (n, 3), dev)
    _check(frame, "frame", torch.float64, (n, 9), dev)
    _check(active, "active", torch.uint8, (n,), dev)
    _check(lists, "lists", torch.int64, (n, VIEWS), dev)
    views = _check_views(views)
    recs, nv = _table(views, dev)
    kstar = torch.empty((n,), dtype=torch.int32, device=dev)
    weight = torch.empty((n,), dtype=torch.float32, device=dev)
    d0 = torch.empty((n,), dtype=torch.float32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    rc = _lib.load().d3d_mesh_refine_match(_ptr(vertices), n, _ptr(frame), _ptr(active), _ptr(lists), _ptr(recs), nv, int(reach), float(step),
                                           float(step if spacing is None else spacing), min_variance(min_contrast), float(min_score),
                                           _ptr(kstar), _ptr(weight), _ptr(d0), _ptr(counts), _stream())
    _lib.check(rc, "d3d_mesh_refine_match")
    return kstar, weight, d0, counts


def relax(weight, d0, active, topology, smooth=DEFAULT_SMOOTH, iterations=DEFAULT_SMOOTH_ITERATIONS):
    """d [n] fp32: the displacement after the screened smoothing (module docstring, Relax)."""
    if not isinstance(weight, torch.Tensor) or weight.device.type != "cuda":
        raise RuntimeError("the mesh is refined on the GPU (no CPU fallback)")
    n, dev = int(weight.shape[0]), weight.device
    _check(weight, "weight", torch.float32, (n,), dev)
    _check(d0, "d0", torch.float32, (n,), dev)
    _check(active, "active", torch.uint8, (n,), dev)
    _check(topology.offset, "offset", torch.int64, (n + 1,), dev)
    out, work = torch.empty_like(d0), torch.empty_like(d0)
    rc = _lib.load().d3d_mesh_refine_relax(_ptr(weight), _ptr(d0), _ptr(active), _ptr(topology.offset), _ptr(topology.nbr), n, float(smooth),
                                           int(iterations), _ptr(work), _ptr(out), _stream())
    _lib.check(rc, "d3d_mesh_refine_relax")
    return out


def apply(vertices, frame, active, d):
    """The moved vertices [n, 3] fp32 (a new tensor): X + d n for the active ones."""
    n, dev = int(vertices.shape[0]), vertices.device
    _check(vertices, "vertices", torch.float32, (n, 3), dev)
    _check(frame, "frame", torch.float64, (n, 9), dev)
    _check(active, "active", torch.uint8, (n,), dev)
    _check(d, "d", torch.float32, (n,), dev)
    out = torch.empty_like(vertices)
    _lib.check(_lib.load().d3d_mesh_refine_apply(_ptr(vertices), n, _ptr(frame), _ptr(active), _ptr(d), _ptr(out), _stream()),
               "d3d_mesh_refine_apply")
    return out


def refine_mesh(vertices, faces, views, step, **settings):
    """(vertices [n, 3] fp32, summary): the mesh refined against `views` (OrthoView records with images) over the scales of the
    settings (check_refine_settings).  summary: {"scales": [{"step", "spacing", "active", "two_views", "matched", "moved",
    "rms_move"} per scale], "vertices": n}.  A mesh without a vertex is returned as it is."""
    s = check_refine_settings(dict(settings, step=step))
    if isinstance(vertices, torch.Tensor) and vertices.dim() == 2 and vertices.shape[0] == 0:
        return vertices, {"scales": [], "vertices": 0}
    vertices, faces, n, m = _mesh_arrays(vertices, faces)
    views = _check_views(views)
    topo = Topology(faces, n)
    step, spacing = s["step"], s["spacing"]
    per_scale = []
    for _ in range(s["scales"]):
        frame, active = vertex_frames(vertices, faces, topo)
        lists = vertex_views(vertices, frame, active, views, step, s["reach"], s["depth_tolerance"], s["views_per_batch"])
        kstar, weight, d0, counts = match(vertices, frame, active, lists, views, step, spacing, s["reach"], s["min_score"], s["min_contrast"])
        d = relax(weight, d0, active, topo, s["smooth"], s["smooth_iterations"])
        vertices = apply(vertices, frame, active, d)
        c = counts.cpu().tolist()
        moved = d[active.bool()].double()
        per_scale.append({"step": step, "spacing": spacing, "active": c[0], "two_views": c[1], "matched": c[2], "moved": c[3],
                          "rms_move": float(moved.pow(2).mean().sqrt()) if moved.numel() else 0.0})
        step, spacing = step * s["scale_step"], spacing * s["scale_step"]
    return vertices, {"scales": per_scale, "vertices": n}


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix="", step_flag=None):
    """The refinement's settings as flags.  The step is --<prefix>step unless step_flag names it (predict's --mesh_refine)."""
    ap.add_argument(step_flag or "--%sstep" % prefix, type=float, default=None, metavar="STEP", dest=prefix + "step",
                    help="refine the mesh against the images: the distance between two hypotheses along the vertex normal, a world "
                         "length > 0 (half the mesh's voxel is a start)")
    ap.add_argument("--%sreach" % prefix, type=int, default=DEFAULT_REACH, help="hypotheses on each side of the vertex (1 .. %d)" % MAX_REACH)
    ap.add_argument("--%sspacing" % prefix, type=float, default=None, help="distance between two points of the 5 x 5 patch (default: the step)")
    ap.add_argument("--%sscales" % prefix, type=int, default=DEFAULT_SCALES, help="passes, each with a finer step (1 .. %d)" % MAX_SCALES)
    ap.add_argument("--%sscale_step" % prefix, type=float, default=DEFAULT_SCALE_STEP, help="the step and the spacing are multiplied by this after a pass")
    ap.add_argument("--%smin_score" % prefix, type=float, default=DEFAULT_MIN_SCORE, help="a vertex whose best correlation is below this stays")
    ap.add_argument("--%smin_contrast" % prefix, type=float, default=DEFAULT_MIN_CONTRAST,
                    help="a patch whose grey varies by less than this (standard deviation, grey levels) is not matched")
    ap.add_argument("--%ssmooth" % prefix, type=float, default=DEFAULT_SMOOTH, help="weight of the neighbours' displacement against the vertex's own (> 0)")
    ap.add_argument("--%ssmooth_iterations" % prefix, type=int, default=DEFAULT_SMOOTH_ITERATIONS, help="Jacobi steps of the smoothing (>= 0)")


def settings_from_args(a, prefix="", depth_tolerance=None, views_per_batch=None):
    """The settings dict of the flags, or None when the step is not given (the stage is off)."""
    g = lambda k: getattr(a, prefix + k)
    if g("step") is None:
        return None
    return {"step": g("step"), "spacing": g("spacing"), "reach": g("reach"), "scales": g("scales"), "scale_step": g("scale_step"),
            "min_score": g("min_score"), "min_contrast": g("min_contrast"), "smooth": g("smooth"), "smooth_iterations": g("smooth_iterations"),
            "depth_tolerance": depth_tolerance, "views_per_batch": views_per_batch}


def check_args(ap, a, prefix="", step_flag=None):
    """The argument errors of the refinement's settings, reported through ap.error."""
    s = settings_from_args(a, prefix)
    if s is None:
        return
    try:
        check_refine_settings(s)
    except ValueError as e:
        ap.error("%s: %s" % (step_flag or "--%sstep" % prefix, e))


def summary_line(info):
    return "; ".join("step %g: %d of %d active vertices matched, %d moved, rms %.4g" % (s["step"], s["matched"], s["active"], s["moved"],
                                                                                          s["rms_move"]) for s in info["scales"])


def main(argv=None):
    ap = argparse.ArgumentParser(description="refine a surface mesh (binary PLY) against predict's depth maps, cameras and images")
    ap.add_argument("--mesh", required=True, help="the mesh (a PLY mesh.write_ply wrote)")
    ap.add_argument("--mvs", required=True, help="predict's output folder: {name}_init.pfm and {name}.txt")
    ap.add_argument("--out", required=True, help="the refined mesh (.ply)")
    ap.add_argument("--image_root", default=None, help="folder the camera files' relative image paths start from")
    ap.add_argument("--depth_tolerance", type=float, default=DEFAULT_TOLERANCE,
                    help="a vertex is hidden from a view when its depth exceeds the view's depth map by more than this share (and the sweep's reach)")
    ap.add_argument("--views_per_batch", type=int, default=None, help="views per call of the view lists (default: all)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.step is None:
        ap.error("--step is required")
    try:
        settings = check_refine_settings(settings_from_args(a, "", a.depth_tolerance, a.views_per_batch))
    except ValueError as e:
        ap.error(str(e))
    if not a.out.endswith(".ply"):
        ap.error("--out must end in .ply")
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is refined on the GPU (no CPU fallback)")
    from .mesh import read_ply, write_ply
    from .ortho import load_mvs_views

    v, f = read_ply(a.mesh)
    views = load_mvs_views(a.mvs, a.image_root)
    out, info = refine_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), views, **settings)
    write_ply(a.out, out, f)
    print("refined mesh %s: %d vertices, %d views; %s" % (a.out, v.shape[0], len(views), summary_line(info)))
    return a.out


if __name__ == "__main__":
    main()
