"""Collapsing the mesh edges shorter than the images resolve (csrc/mesh_collapse.hip), off by default.

The marching-tetrahedra extraction emits many sliver triangles whose edges are shorter than a pixel in every view: they cost every
later stage work for nothing the images can show.  The decimation (§4.14) removes edges by quadric error down to a face count chosen
by hand; this stage removes the edges shorter than min_edge pixels in every view that sees them and stops by itself.  It is the
other half of the subdivision (§4.23), which splits the edges longer than max_edge pixels.  The rule is this project's own; it
does not claim to match OpenMVS's RefineMesh (nEnsureEdgeSize).  All arithmetic is fp64 without contraction, rounded to fp32 only
where said.  There are no float atomics (the winners are taken by the decimation's 64-bit integer atomicMin).

1. Input.  vertices [n,3] fp32 and faces [m,3] int32, every face with three distinct indices in 0 .. n - 1 (anything else is
   refused, as decimation, hole closing and subdivision refuse it).  views: mesh.MeshView records (K, E = Tcw, depth [H,W] fp32;
   the confidence is not read).  min_edge is a finite pixel length > 0 and has no default.  max_edge is a finite pixel length >=
   2 min_edge; its default, 4 min_edge, is a setting, not a measurement.  The factor 2 is derived, not tuned: subdividing an edge
   longer than max_edge leaves halves of about max_edge / 2, and those must not be short again.
2. Edges.  The undirected edges a < b of the mesh, numbered e = 0, 1, .. in (a, b) lexicographic order, as
   d3d_mesh_decimate_edges numbers them (subdivide.edge_list's list).
3. Measure.  subdivide.measure_edges, unchanged (§4.23 rule 3, with its depth tolerance, 0.01 by default, and its max-merge over
   batches): the largest squared pixel length of the edge over the views that see both of its ends, 0 when no view does.  Edge
   e is short when 0 < measure[e] < min_edge^2.  Geometry no view sees is left alone however small it is.
4. Candidates.  One per short edge with a free end; `fixed` is mesh.adjacency's flag (a vertex on a boundary or non-manifold
   edge, or on no face), so the boundary never moves.  With one end fixed that end survives and the target t is its position.
   With both free, a survives and t = fp32((fp64(x_a) + fp64(x_b)) * 0.5) per component, the subdivision's midpoint.  With
   N(v) the neighbours of v, the candidate is valid when all four hold:
   (1) the decimation's link condition: N(a) and N(b) share exactly two vertices;
   (2) |N(a)| + |N(b)| - 4 >= 3;
   (3) no face at a or b that does not hold both ends turns over or loses its area when the end moves to t: with the normal
       (p1 - p0) x (p2 - p0) in the face's corner order, old normal . new normal > 0, the dot product summed left to right
       (exactly the decimation's test);
   (4) the length guard: with d = x_b - x_a, L2 = (dx dx + dy dy) + dz dz and s = measure[e] / L2, every w in (N(a) u N(b)) \\
       {a, b} has (|t - x_w|^2) s <= max_edge^2, the squared distance summed the same way from the fp32 t; a NaN fails.  It
       estimates the pixel length of the edges the survivor will have from the collapsing edge's own pixels per world unit, so
       it needs no view, and it keeps the stage from making the edges the subdivision would split again.
   key = (bits(fp32(measure[e])) << 32) | (e * 2654435761 mod 2^32): the shortest edge first, the hash spreading ties.  key = -1
   when the edge is not short, has both ends fixed, is not valid, or lies past the edge count; target [E,3] fp32 is t, and 0
   wherever the key is -1.
5. Winners and output.  The decimation's rules 7 and 8 with every valid candidate eligible (the threshold is the largest int64;
   there is no select pass): a candidate claims a, b and all their neighbours with the 64-bit minimum of the keys and wins when it
   reads its own key back everywhere; the survivor of a winner moves to t, the other end is remapped to it, the faces that lose
   an edge are dropped, the others keep their order, and the vertices no face uses any more are dropped with the indices
   renumbered in increasing order.  Winners have disjoint neighbourhoods, so validity judged on the round's input mesh holds for
   all of them.
6. Rounds.  The step repeats on its result with a fresh adjacency, edge list and measure, up to `rounds` times (1 .. 64; the
   default 16 is a setting, not a measurement), and stops early when a round has no winner.  That costs one device-to-host read
   of the counts per round.
The result is a function of the input arrays and the set of views: the same bits for any view order and any views_per_batch.
Permuting the face list gives the same vertices bit for bit and the same set of faces: nothing in the rule sums in face order,
and vertices are renumbered by index.  (Rotating a face's corners is not covered: test (3) takes its normals in corner order.)
There is no CPU fallback.

    python -m deep3d_aerial_amd.collapse --mesh IN.ply --mvs MVS --out OUT.ply --min_edge PX [--max_edge PX2] [--rounds R]
        [--depth_tolerance T] [--views_per_batch N]
"""
import argparse
import ctypes
import math

import torch

from . import _geom, _lib
from ._geom import ptr as _ptr, stream as _stream
from .mesh import _check_views, _decimate_arrays

DEFAULT_TOLERANCE = 0.01
DEFAULT_ROUNDS = 16
MAX_ROUNDS = 64
DEFAULT_MAX_EDGE_FACTOR = 4.0   # max_edge = 4 min_edge unless given: a setting, not a measurement
I64_MAX = (1 << 63) - 1
_KEYS = ("min_edge", "max_edge", "rounds", "depth_tolerance", "views_per_batch")


def _pixels(settings, key, what):
    try:
        x = float(settings[key])
    except (TypeError, ValueError):
        raise ValueError("collapse %s %r must be %s" % (key, settings[key], what))
    if not math.isfinite(x):
        raise ValueError("collapse %s %r must be %s" % (key, settings[key], what))
    return x


def check_collapse_settings(settings):
    """The settings dict checked and completed: {"min_edge", "max_edge", "rounds", "depth_tolerance", "views_per_batch"}.
    min_edge has no default; max_edge defaults to 4 min_edge."""
    unknown = set(settings) - set(_KEYS)
    if unknown:
        raise ValueError("collapse: unknown settings %s" % sorted(unknown))
    if settings.get("min_edge") is None:
        raise ValueError("collapse needs min_edge (the shortest edge left alone, a pixel length > 0)")
    g = lambda k, d: d if settings.get(k) is None else settings[k]
    min_edge = _pixels(settings, "min_edge", "a finite pixel length > 0")
    if not min_edge > 0:
        raise ValueError("collapse min_edge %r must be a finite pixel length > 0" % (settings["min_edge"],))
    max_edge = DEFAULT_MAX_EDGE_FACTOR * min_edge if settings.get("max_edge") is None else _pixels(settings, "max_edge", "a finite pixel length")
    if not (math.isfinite(max_edge) and max_edge >= 2 * min_edge):
        raise ValueError("collapse max_edge %r must be a finite pixel length >= 2 min_edge (%r): the halves of a subdivided edge must not "
                         "be short again" % (max_edge, 2 * min_edge))
    rounds = g("rounds", DEFAULT_ROUNDS)
    try:
        whole = int(rounds) == rounds
    except (TypeError, ValueError):
        whole = False
    if not whole or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError("collapse rounds %r must be an integer in 1 .. %d" % (rounds, MAX_ROUNDS))
    tol = float(g("depth_tolerance", DEFAULT_TOLERANCE))
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError("collapse depth_tolerance %r must be finite and >= 0" % (settings.get("depth_tolerance"),))
    return {"min_edge": min_edge, "max_edge": max_edge, "rounds": int(rounds), "depth_tolerance": tol,
            "views_per_batch": _geom.check_views_per_batch(settings.get("views_per_batch"))}


def candidates(vertices, faces, csr, incidence, edges, n_edges, measure, min_edge, max_edge):
    """Rule 4 on the device: (target [E,3] fp32, key [E] int64) of the edges [E,2] (n_edges of them; subdivide.edge_list) with
    their measure [E] fp64 (subdivide.measure_edges).  csr: mesh.adjacency's (offset, nbr, fixed); incidence:
    mesh.face_incidence's (face_offset, face_index).  No read."""
    s = check_collapse_settings({"min_edge": min_edge, "max_edge": max_edge})
    n, m, emax = int(vertices.shape[0]), int(faces.shape[0]), int(edges.shape[0])
    dev = vertices.device
    if not (isinstance(measure, torch.Tensor) and measure.dtype == torch.float64 and tuple(measure.shape) == (emax,) and measure.device == dev
            and measure.is_contiguous()):
        raise ValueError("measure must be a contiguous [%d] float64 tensor on %s" % (emax, dev))
    offset, nbr, fixed = csr
    foff, finc = incidence
    target = torch.empty((max(emax, 1), 3), dtype=torch.float32, device=dev)
    key = torch.empty((max(emax, 1),), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().d3d_mesh_collapse_candidates(_ptr(vertices), n, _ptr(faces), m, _ptr(offset), _ptr(nbr), _ptr(fixed), _ptr(foff),
                                                        _ptr(finc), _ptr(edges), _ptr(n_edges), emax, _ptr(measure), s["min_edge"], s["max_edge"],
                                                        _ptr(target), _ptr(key), _stream()), "d3d_mesh_collapse_candidates")
    return target[:emax], key[:emax]


def _record(edges=0, short=0, valid=0, winners=0, vertices_out=0, faces_out=0):
    return {"edges": edges, "short": short, "valid": valid, "winners": winners, "vertices_out": vertices_out, "faces_out": faces_out}


def topology(faces, n_vertices):
    """What a round reads of the connectivity, on the device: {"offset", "nbr", "fixed" (mesh.adjacency), "face_offset",
    "face_index" (mesh.face_incidence), "edges" [3 m, 2] int32 and "n_edges" [1] int64 (rule 2's list: subdivide.edge_list; the rows
    from the edge count on are 0), "counts" [3] int64: 0 for the winners, the kept faces and the kept vertices the later passes
    count}.  "nbr" and "face_index" are defined up to offset[n] and face_offset[n], as in mesh.adjacency and
    mesh.face_incidence."""
    from . import subdivide as _subdivide
    from .mesh import adjacency, face_incidence

    n = int(n_vertices)
    offset, nbr, fixed = adjacency(faces, n)
    foff, finc = face_incidence(faces, n)
    edges, n_edges = _subdivide.edge_list(faces, n, csr=(offset, nbr, fixed))
    return {"offset": offset, "nbr": nbr, "fixed": fixed, "face_offset": foff, "face_index": finc, "edges": edges, "n_edges": n_edges,
            "counts": torch.zeros((3,), dtype=torch.int64, device=faces.device)}


def _count(counts, i):
    return ctypes.c_void_p(counts.data_ptr() + 8 * i)


def claim_apply(vertices, topo, target, key):
    """Rule 5's winners, by the decimation's claim and apply passes with every valid key eligible: (moved [n,3] fp32: the vertices
    with the survivors at their targets, remap [n] int32, win [E] uint8, claim [n] int64); topo["counts"][0] gets the winners."""
    lib = _lib.load()
    n, emax = int(vertices.shape[0]), int(topo["edges"].shape[0])
    dev = vertices.device
    st = _stream()
    offset, nbr, fixed, edges, n_edges, counts = (topo[k] for k in ("offset", "nbr", "fixed", "edges", "n_edges", "counts"))
    threshold = torch.full((1,), I64_MAX, dtype=torch.int64, device=dev)
    claim = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_decimate_claim(_ptr(offset), _ptr(nbr), n, _ptr(edges), _ptr(key), _ptr(n_edges), emax, _ptr(threshold),
                                           _ptr(claim), _count(counts, 0), st), "d3d_mesh_decimate_claim")
    moved = torch.empty_like(vertices)
    remap = torch.empty((n,), dtype=torch.int32, device=dev)
    win = torch.empty((emax,), dtype=torch.uint8, device=dev)
    _lib.check(lib.d3d_mesh_decimate_apply(_ptr(vertices), n, _ptr(offset), _ptr(nbr), _ptr(fixed), _ptr(edges), _ptr(key), _ptr(target),
                                           _ptr(n_edges), emax, _ptr(threshold), _ptr(claim), _ptr(moved), _ptr(remap), _ptr(win),
                                           _count(counts, 0), st), "d3d_mesh_decimate_apply")
    return moved, remap, win, claim


def faces_compact(moved, faces, remap, counts):
    """Rule 5's output, by the decimation's faces pass and d3d_mesh_compact: (vertices [n,3], faces [m,3]) of which the first
    counts[2] and counts[1] rows hold the mesh after the round (the counts are still on the device).  The vertex rows from
    counts[2] on are never written; the face rows from counts[1] on are 0."""
    lib = _lib.load()
    n, m = int(moved.shape[0]), int(faces.shape[0])
    dev = moved.device
    st = _stream()
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_faces_scratch_bytes, m, device=dev)
    out_faces = torch.zeros((m, 3), dtype=torch.int32, device=dev)   # rows past the kept ones stay 0: a valid index
    referenced = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_mesh_decimate_faces(_ptr(faces), m, n, _ptr(remap), _ptr(scratch), nbytes, _ptr(out_faces), _ptr(referenced),
                                           _count(counts, 1), st), "d3d_mesh_decimate_faces")
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_scan_scratch_bytes, n, device=dev)
    renum = torch.empty((n,), dtype=torch.int32, device=dev)
    out_v = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _lib.check(lib.d3d_mesh_compact(_ptr(moved), n, _ptr(out_faces), m, _ptr(referenced), _ptr(scratch), nbytes, _ptr(renum), _ptr(out_v),
                                    _count(counts, 2), st), "d3d_mesh_compact")
    return out_v, out_faces


def _round(vertices, faces, n, m, views, s, detail=None):
    """collapse_round on arrays and settings already checked."""
    from . import subdivide as _subdivide

    if n == 0 or m == 0:
        return vertices, faces, _record(vertices_out=n, faces_out=m)
    topo = topology(faces, n)
    edges, counts = topo["edges"], topo["counts"]
    measure = _subdivide.measure_edges(vertices, edges, topo["n_edges"], views, s["depth_tolerance"], s["views_per_batch"])
    target, key = candidates(vertices, faces, (topo["offset"], topo["nbr"], topo["fixed"]), (topo["face_offset"], topo["face_index"]), edges,
                             topo["n_edges"], measure, s["min_edge"], s["max_edge"])
    moved, remap, win, claim = claim_apply(vertices, topo, target, key)
    out_v, out_faces = faces_compact(moved, faces, remap, counts)
    short = ((measure > 0) & (measure < s["min_edge"] * s["min_edge"])).sum().reshape(1)
    valid = (key >= 0).sum().reshape(1)
    ne, nw, mk, nk, n_short, n_valid = torch.cat([topo["n_edges"], counts, short, valid]).cpu().tolist()   # the round's one read
    if detail is not None:
        detail.update(offset=topo["offset"], nbr=topo["nbr"][:2 * ne], fixed=topo["fixed"], face_offset=topo["face_offset"],
                      face_index=topo["face_index"], edges=edges[:ne], n_edges=ne, measure=measure[:ne], target=target[:ne], key=key[:ne],
                      claim=claim, win=win[:ne], remap=remap)
    if nw == 0:
        return vertices, faces, _record(ne, n_short, n_valid, 0, n, m)
    return out_v[:nk], out_faces[:mk], _record(ne, n_short, n_valid, nw, nk, mk)


def collapse_round(vertices, faces, views, min_edge, max_edge, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, detail=None):
    """One round (rules 2-5): (vertices, faces, record); with no winner the input tensors come back.  record: {"edges", "short",
    "valid", "winners", "vertices_out", "faces_out"}.  detail (a dict) gets every pass's output: offset, nbr, fixed, face_offset,
    face_index, edges [E,2], n_edges, measure [E], target [E,3], key [E] (-1: no candidate), claim [n], win [E], remap [n].  One
    device-to-host read after the checks of the input."""
    s = check_collapse_settings({"min_edge": min_edge, "max_edge": max_edge, "depth_tolerance": depth_tolerance, "views_per_batch": views_per_batch})
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "collapse")
    views = _check_views(views, vertices.device)
    return _round(vertices, faces, n, m, views, s, detail)


def collapse(vertices, faces, views, min_edge, max_edge=None, rounds=DEFAULT_ROUNDS, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None,
             info=None):
    """The mesh with the edges shorter than min_edge pixels in every view that sees them collapsed, over up to `rounds` rounds, on
    the device: (vertices, faces).  With nothing to collapse the input tensors come back as they are.  info (a dict) gets
    {"edges", "short", "valid", "winners": one number per round, "rounds": the rounds run, "hit_max_rounds": the last allowed round
    still had a winner, "faces_in", "faces_out", "vertices_out"}."""
    s = check_collapse_settings({"min_edge": min_edge, "max_edge": max_edge, "rounds": rounds, "depth_tolerance": depth_tolerance,
                                 "views_per_batch": views_per_batch})
    v, f, n, m = _decimate_arrays(vertices, faces, "collapse")
    views = _check_views(views, v.device)
    rec = {"edges": [], "short": [], "valid": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces_in": m}
    won = False
    for k in range(s["rounds"] if n and m else 0):
        v, f, r = _round(v, f, int(v.shape[0]), int(f.shape[0]), views, s)
        rec["rounds"] += 1
        for key in ("edges", "short", "valid", "winners"):
            rec[key].append(r[key])
        if r["winners"] == 0:
            break
        won = True
        rec["hit_max_rounds"] = k + 1 == s["rounds"]
    rec.update(faces_out=int(f.shape[0]) if won else m, vertices_out=int(v.shape[0]) if won else n)
    if info is not None:
        info.update(rec)
    if not won:
        return vertices, faces
    return v, f


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix="", edge_flag=None, tolerance=True):
    """The collapse's settings as flags.  The short length is --<prefix>min_edge unless edge_flag names it (the mesh stage's
    --collapse, predict's --mesh_collapse); tolerance=False leaves --<prefix>depth_tolerance out."""
    ap.add_argument(edge_flag or "--%smin_edge" % prefix, type=float, default=None, metavar="PX", dest=prefix + "min_edge",
                    help="collapse the mesh: remove every edge shorter than PX pixels (> 0) in every view that sees it")
    ap.add_argument("--%smax_edge" % prefix, type=float, default=None, metavar="PX2",
                    help="no collapse may leave an edge estimated longer than PX2 pixels (>= 2 PX; default 4 PX, or the subdivision's "
                         "length when the mesh stage runs both)")
    ap.add_argument("--%srounds" % prefix, type=int, default=DEFAULT_ROUNDS, metavar="R",
                    help="collapse rounds, each taking the independent short edges (1 .. %d)" % MAX_ROUNDS)
    if tolerance:
        ap.add_argument("--%sdepth_tolerance" % prefix, type=float, default=DEFAULT_TOLERANCE,
                        help="an endpoint is hidden from a view when its depth exceeds the view's depth map by more than this share")


def settings_from_args(a, prefix="", views_per_batch=None):
    """The settings dict of the flags, or None when the short length is not given (the stage is off)."""
    g = lambda k: getattr(a, prefix + k)
    if g("min_edge") is None:
        return None
    return {"min_edge": g("min_edge"), "max_edge": g("max_edge"), "rounds": g("rounds"),
            "depth_tolerance": getattr(a, prefix + "depth_tolerance", DEFAULT_TOLERANCE), "views_per_batch": views_per_batch}


def check_args(ap, a, prefix="", edge_flag=None):
    """The argument errors of the collapse's settings, reported through ap.error."""
    s = settings_from_args(a, prefix)
    if s is None:
        return
    try:
        check_collapse_settings(s)
    except ValueError as e:
        ap.error("%s: %s" % (edge_flag or "--%smin_edge" % prefix, e))


def summary_line(info):
    per = "; ".join("round %d: %d of %d edges short, %d valid, %d collapsed" % (i + 1, info["short"][i], info["edges"][i], info["valid"][i], w)
                    for i, w in enumerate(info["winners"]))
    if not per:
        return per
    return per + "; %d -> %d faces, %d vertices%s" % (info["faces_in"], info["faces_out"], info["vertices_out"],
                                                     "; reached the round limit" if info["hit_max_rounds"] else "")


def main(argv=None):
    ap = argparse.ArgumentParser(description="collapse the edges of a surface mesh (binary PLY) that predict's views cannot resolve")
    ap.add_argument("--mesh", required=True, help="the mesh (a PLY mesh.write_ply wrote)")
    ap.add_argument("--mvs", required=True, help="predict's output folder: {name}_init.pfm, {name}_prob.pfm and {name}.txt")
    ap.add_argument("--out", required=True, help="the collapsed mesh (.ply)")
    ap.add_argument("--views_per_batch", type=int, default=None, help="views per call of the measure (default: all)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.min_edge is None:
        ap.error("--min_edge is required")
    try:
        s = check_collapse_settings(settings_from_args(a, "", a.views_per_batch))
    except ValueError as e:
        ap.error(str(e))
    if not a.out.endswith(".ply"):
        ap.error("--out must end in .ply")
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is collapsed on the GPU (no CPU fallback)")
    from .mesh import load_mvs_views, read_ply, write_ply

    v, f = read_ply(a.mesh)
    views = load_mvs_views(a.mvs)
    info = {}
    out_v, out_f = collapse(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), views, info=info, **s)
    write_ply(a.out, out_v, out_f)
    print("collapsed mesh %s: %d -> %d vertices, %d -> %d faces, %d views; %s" % (a.out, v.shape[0], out_v.shape[0], f.shape[0], out_f.shape[0],
                                                                                 len(views), summary_line(info) or "nothing to collapse"))
    return a.out


if __name__ == "__main__":
    main()
