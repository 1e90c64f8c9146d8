"""Subdividing the surface mesh where the images outresolve it (csrc/mesh_subdivide.hip), off by default.

The mesh stage's resolution is the TSDF voxel's; decimation removes vertices and the refinement only moves them.  This stage adds
them: every mesh edge whose projection is longer than max_edge pixels in some view that sees it is split at its midpoint, over a
few rounds, with conforming face splits.  It is the complement of the decimation (§4.14).  The rule is this project's own;
it does not claim to match OpenMVS's RefineMesh subdivision (nMaxFaceArea, nEnsureEdgeSize).  All arithmetic is fp64 without
contraction, rounded to fp32 only where said.  There are no float atomics and no integer atomics either.

1. Input.  vertices [n,3] fp32 and faces [m,3] int32, every face with three distinct indices in 0 .. n - 1 (anything else is
   refused, as decimation and hole closing refuse it).  views: mesh.MeshView records (K, E = Tcw, depth [H,W] fp32; the
   confidence is not read).  max_edge is a pixel length >= 1 and has no default.
2. Edges.  The undirected edges a < b of the mesh, numbered e = 0, 1, .. in (a, b) lexicographic order, as
   d3d_mesh_decimate_edges numbers them.
3. Measure.  A view sees an endpoint X under ortho's candidate test, restated: p = R X + t, q = K p, each row summed left to
   right, p2 > 0 and q2 > 0; u = q0 / q2, v = q1 / q2 with 0 <= u <= W-1 and 0 <= v <= H-1; the depth D at pixel
   (floor(v + 0.5), floor(u + 0.5)) is finite and > 0; p2 <= D (1 + depth_tolerance), depth_tolerance 0.01 by default.  A view
   that sees both endpoints contributes l2 = (ua - ub)^2 + (va - vb)^2; a non-finite l2 rejects the view.  The edge's measure is
   the maximum l2 over the views, 0 when no view sees both ends.  A maximum does not depend on view order, batching or rank
   split: the measure array [max_edges] fp64 is max-merged across calls (measure_edges(..., measure=...)), as the refinement's
   vertex_views min-merges its lists.
4. Mark.  The midpoint of an edge is fp32((fp64(x_a) + fp64(x_b)) * 0.5) per component.  An edge is split when its measure >
   max_edge^2 and its midpoint differs from both ends.  The new vertex of a split edge has index n + the exclusive rank of the
   edge among the split edges, in edge order, so the numbering does not depend on the face order.
5. Faces.  Take face (v0, v1, v2) with edges e_i = (v_i, v_{i+1}) and midpoints m_i.  Its children replace it at its place in the
   face order (groups in input face order, children in the order given), with the winding kept:
   * no edge split: (v0, v1, v2);
   * only e_i split, (a, b, c) = (v_i, v_{i+1}, v_{i+2}): (a, m_i, c), (m_i, b, c);
   * only e_i unsplit, (a, b, c) alike, p = m_{i+1}, q = m_{i+2}: first (p, c, q); then the quad a, b, p, q is cut by the shorter
     of its diagonals a-p and b-q, the squared length taken in fp64 as (dx^2 + dy^2) + dz^2 on the fp32 positions; a-p gives
     (a, b, p), (a, p, q) and b-q gives (a, b, q), (b, p, q); on a tie the diagonal that starts at the smaller of the indices a
     and b is taken;
   * all three split: (v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2).
   Midpoints are shared per edge, so the result is conforming on manifold, boundary and non-manifold edges alike.  Boundary edges
   may be split.
6. Output.  The input vertices come first and unchanged, then the midpoints.
7. Rounds.  The step repeats on its result, with a fresh adjacency, edge list and measure, up to `rounds` times (1 .. 8; the
   default 4 is a setting, not a measurement), and stops early when a round splits nothing.  That costs one device-to-host read of the
   totals per round, as plan_holes does.  A result with n + splits >= 2^31 or 6 x faces_out >= 2^31 is refused (ValueError)
   before anything is emitted.
The result is a function of the input arrays and the set of views.  Permuting the faces or rotating their corners gives the same
vertices bit for bit and the same set of faces.  There is no CPU fallback.

    python -m deep3d_aerial_amd.subdivide --mesh IN.ply --mvs MVS --out OUT.ply --max_edge PX [--rounds R] [--depth_tolerance T]
        [--views_per_batch N]
"""
import argparse
import ctypes
import math

import torch

from . import _geom, _lib
from ._geom import batches as _batches, ptr as _ptr, stream as _stream
from .mesh import _check_views, _decimate_arrays

DEFAULT_TOLERANCE = 0.01
DEFAULT_ROUNDS = 4
MAX_ROUNDS = 8
_KEYS = ("max_edge", "rounds", "depth_tolerance", "views_per_batch")


def check_subdivide_settings(settings):
    """The settings dict checked and completed: {"max_edge", "rounds", "depth_tolerance", "views_per_batch"}.  max_edge has no
    default."""
    unknown = set(settings) - set(_KEYS)
    if unknown:
        raise ValueError("subdivide: unknown settings %s" % sorted(unknown))
    if settings.get("max_edge") is None:
        raise ValueError("subdivide needs max_edge (the longest edge left alone, a pixel length >= 1)")
    g = lambda k, d: d if settings.get(k) is None else settings[k]
    try:
        max_edge = float(settings["max_edge"])
    except (TypeError, ValueError):
        raise ValueError("subdivide max_edge %r must be a pixel length >= 1" % (settings["max_edge"],))
    if not (math.isfinite(max_edge) and max_edge >= 1):
        raise ValueError("subdivide max_edge %r must be a finite pixel length >= 1" % (settings["max_edge"],))
    rounds = g("rounds", DEFAULT_ROUNDS)
    try:
        whole = int(rounds) == rounds
    except (TypeError, ValueError):
        whole = False
    if not whole or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError("subdivide rounds %r must be an integer in 1 .. %d" % (rounds, MAX_ROUNDS))
    tol = float(g("depth_tolerance", DEFAULT_TOLERANCE))
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError("subdivide depth_tolerance %r must be finite and >= 0" % (settings.get("depth_tolerance"),))
    return {"max_edge": max_edge, "rounds": int(rounds), "depth_tolerance": tol,
            "views_per_batch": _geom.check_views_per_batch(settings.get("views_per_batch"))}


def check_sizes(n_vertices, splits, faces_out):
    """The int32 refusal of rule 7, before anything is emitted."""
    if n_vertices + splits >= 1 << 31 or 6 * faces_out >= 1 << 31:
        raise ValueError("%d + %d vertices, %d faces after the split: more than int32 indexes (n + splits < 2^31, 6 faces < 2^31)"
                         % (n_vertices, splits, faces_out))


def edge_list(faces, n_vertices, csr=None):
    """(edges [3 m, 2] int32, n_edges [1] int64) on the device: rule 2's list (d3d_mesh_decimate_edges over mesh.adjacency); the rows
    from n_edges on are not written.  csr: mesh.adjacency(faces, n_vertices) when the caller has it."""
    from .mesh import adjacency

    lib = _lib.load()
    n, m = int(n_vertices), int(faces.shape[0])
    dev = faces.device
    offset, nbr, _ = csr if csr is not None else adjacency(faces, n)
    emax = 3 * m
    edges = torch.zeros((max(emax, 1), 2), dtype=torch.int32, device=dev)
    n_edges = torch.zeros((1,), dtype=torch.int64, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_decimate_edges_scratch_bytes, n, device=dev)
    _lib.check(lib.d3d_mesh_decimate_edges(_ptr(offset), _ptr(nbr), n, _ptr(scratch), nbytes, emax, _ptr(edges), _ptr(n_edges), _stream()),
               "d3d_mesh_decimate_edges")
    return edges[:emax], n_edges


def _check_edges(vertices, edges, n_edges):
    if not (isinstance(vertices, torch.Tensor) and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3):
        raise ValueError("vertices must be [n,3] float32")
    dev = vertices.device
    if dev.type != "cuda":
        raise RuntimeError("the mesh is subdivided on the GPU (no CPU fallback); got %s" % dev)
    if not (isinstance(edges, torch.Tensor) and edges.dtype == torch.int32 and edges.dim() == 2 and edges.shape[1] == 2 and edges.device == dev
            and edges.is_contiguous()):
        raise ValueError("edges must be a contiguous [E,2] int32 tensor on %s" % dev)
    if not (isinstance(n_edges, torch.Tensor) and n_edges.dtype == torch.int64 and n_edges.numel() == 1 and n_edges.device == dev):
        raise ValueError("n_edges must be one int64 on %s (edge_list's count)" % dev)
    return vertices.contiguous(), int(vertices.shape[0]), int(edges.shape[0])


def measure_edges(vertices, edges, n_edges, views, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, measure=None):
    """Rule 3: measure [E] fp64, the largest squared pixel length of every edge over `views`, max-merged into `measure` when one
    is given (all 0 at first): calls over any split of the views, in any order, give the same array."""
    vertices, n, emax = _check_edges(vertices, edges, n_edges)
    dev = vertices.device
    tol = check_subdivide_settings({"max_edge": 1.0, "depth_tolerance": depth_tolerance})["depth_tolerance"]
    vpb = _geom.check_views_per_batch(views_per_batch)
    views = _check_views(views, dev)
    if measure is None:
        measure = torch.zeros((emax,), dtype=torch.float64, device=dev)
    elif not (isinstance(measure, torch.Tensor) and measure.dtype == torch.float64 and tuple(measure.shape) == (emax,) and measure.device == dev
              and measure.is_contiguous()):
        raise ValueError("measure must be a contiguous [%d] float64 tensor on %s" % (emax, dev))
    if emax == 0 or n == 0:
        return measure
    from .mesh import _records

    lib = _lib.load()
    for batch in _batches(views, vpb):
        recs = _records(batch, dev)
        _lib.check(lib.d3d_mesh_subdivide_measure(_ptr(vertices), n, _ptr(edges), _ptr(n_edges), emax, _ptr(recs), len(batch), tol, _ptr(measure),
                                                  _stream()), "d3d_mesh_subdivide_measure")
    return measure


def plan(vertices, faces, edges, n_edges, measure, max_edge):
    """Rules 4 and 5's counts, on the device: {"mark", "rank" [E] int32, "midpoint" [E,3] fp32, "face_edge" [m,3] int32,
    "child_count", "child_offset" [m] int32, "totals" [2] int64 (the split edges, the faces after the split)}.  No read."""
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "subdivision")
    _, _, emax = _check_edges(vertices, edges, n_edges)
    max_edge = check_subdivide_settings({"max_edge": max_edge})["max_edge"]
    dev = vertices.device
    if not (isinstance(measure, torch.Tensor) and measure.dtype == torch.float64 and tuple(measure.shape) == (emax,) and measure.device == dev):
        raise ValueError("measure must be a [%d] float64 tensor on %s" % (emax, dev))
    lib = _lib.load()
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_subdivide_scratch_bytes, m, emax, device=dev)
    if nbytes == 0:
        raise ValueError("%d faces, %d edges: out of range" % (m, emax))
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    E, M = max(emax, 1), max(m, 1)
    d = {"mark": i32(E), "rank": i32(E), "midpoint": torch.empty((E, 3), dtype=torch.float32, device=dev), "face_edge": i32(M, 3),
         "child_count": i32(M), "child_offset": i32(M), "totals": torch.empty((2,), dtype=torch.int64, device=dev)}
    _lib.check(lib.d3d_mesh_subdivide_plan(_ptr(vertices), n, _ptr(faces), m, _ptr(edges), _ptr(n_edges), emax, _ptr(measure.contiguous()), max_edge,
                                           _ptr(scratch), nbytes, _ptr(d["mark"]), _ptr(d["rank"]), _ptr(d["midpoint"]), _ptr(d["face_edge"]),
                                           _ptr(d["child_count"]), _ptr(d["child_offset"]), _ptr(d["totals"]), _stream()),
               "d3d_mesh_subdivide_plan")
    for k in ("mark", "rank", "midpoint"):
        d[k] = d[k][:emax]
    for k in ("face_edge", "child_count", "child_offset"):
        d[k] = d[k][:m]
    return d


def emit(vertices, faces, n_edges, p, splits, faces_out):
    """Rules 5 and 6 with plan's dict and its totals as the host read them: (vertices [n + splits, 3], faces [faces_out, 3])."""
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "subdivision")
    splits, faces_out = int(splits), int(faces_out)
    check_sizes(n, splits, faces_out)
    dev = vertices.device
    emax = int(p["mark"].shape[0])
    out_v = torch.empty((n + splits, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((faces_out, 3), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().d3d_mesh_subdivide_emit(_ptr(vertices), n, _ptr(faces), m, _ptr(n_edges), emax, _ptr(p["mark"]), _ptr(p["rank"]),
                                                   _ptr(p["midpoint"]), _ptr(p["face_edge"]), _ptr(p["child_offset"]), splits, faces_out,
                                                   _ptr(out_v), _ptr(out_f), _stream()), "d3d_mesh_subdivide_emit")
    return out_v, out_f


def subdivide_round(vertices, faces, views, max_edge, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, detail=None):
    """One round (rules 2-6): (vertices, faces, record); with nothing to split the input tensors come back.  record: {"edges",
    "seen" (measure > 0), "split", "vertices_out", "faces_out", "longest_px"}.  detail (a dict) gets every pass's output: edges
    [E,2], n_edges, measure [E] and plan's arrays, cut to the edge count.  One device-to-host read."""
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "subdivision")
    if n == 0 or m == 0:
        return vertices, faces, {"edges": 0, "seen": 0, "split": 0, "vertices_out": n, "faces_out": m, "longest_px": 0.0}
    edges, n_edges = edge_list(faces, n)
    measure = measure_edges(vertices, edges, n_edges, views, depth_tolerance, views_per_batch)
    p = plan(vertices, faces, edges, n_edges, measure, max_edge)
    seen = (measure > 0).sum().reshape(1)
    longest = measure.max().reshape(1).view(torch.int64)
    splits, faces_out, ne, n_seen, bits = torch.cat([p["totals"], n_edges, seen, longest]).cpu().tolist()   # the round's one read
    longest_px = math.sqrt(ctypes.c_double.from_buffer(ctypes.c_int64(bits)).value)
    rec = {"edges": ne, "seen": n_seen, "split": splits, "vertices_out": n + splits, "faces_out": faces_out, "longest_px": longest_px}
    if detail is not None:
        detail.update(edges=edges[:ne], n_edges=ne, measure=measure[:ne], mark=p["mark"][:ne], rank=p["rank"][:ne], midpoint=p["midpoint"][:ne],
                      face_edge=p["face_edge"], child_count=p["child_count"], child_offset=p["child_offset"], totals=p["totals"])
    if splits == 0:
        return vertices, faces, rec
    out_v, out_f = emit(vertices, faces, n_edges, p, splits, faces_out)
    return out_v, out_f, rec


def subdivide(vertices, faces, views, max_edge, rounds=DEFAULT_ROUNDS, depth_tolerance=DEFAULT_TOLERANCE, views_per_batch=None, info=None):
    """The mesh with every edge longer than max_edge pixels in a view that sees it split, over up to `rounds` rounds, on the device:
    (vertices, faces), the input vertices first and unchanged.  With nothing to split the input tensors come back as they are.
    info (a dict) gets {"rounds": [subdivide_round's record per round], "stopped_early": a round split nothing, "vertices",
    "faces": the result's sizes}."""
    s = check_subdivide_settings({"max_edge": max_edge, "rounds": rounds, "depth_tolerance": depth_tolerance, "views_per_batch": views_per_batch})
    v, f, n, m = _decimate_arrays(vertices, faces, "subdivision")
    views = _check_views(views, v.device)
    per_round, early = [], False
    for _ in range(s["rounds"] if n and m else 0):
        v, f, rec = subdivide_round(v, f, views, s["max_edge"], s["depth_tolerance"], s["views_per_batch"])
        per_round.append(rec)
        if rec["split"] == 0:
            early = True
            break
    if info is not None:
        info.update(rounds=per_round, stopped_early=early, vertices=int(v.shape[0]), faces=int(f.shape[0]))
    if not any(r["split"] for r in per_round):
        return vertices, faces
    return v, f


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix="", edge_flag=None, tolerance=True):
    """The subdivision's settings as flags.  The edge length is --<prefix>max_edge unless edge_flag names it (the mesh stage's
    --subdivide, predict's --mesh_subdivide); tolerance=False leaves --<prefix>depth_tolerance out."""
    ap.add_argument(edge_flag or "--%smax_edge" % prefix, type=float, default=None, metavar="PX", dest=prefix + "max_edge",
                    help="subdivide the mesh: split every edge longer than PX pixels (>= 1) in a view that sees it")
    ap.add_argument("--%srounds" % prefix, type=int, default=DEFAULT_ROUNDS, metavar="R",
                    help="subdivision rounds, each halving the edges still too long (1 .. %d)" % MAX_ROUNDS)
    if tolerance:
        ap.add_argument("--%sdepth_tolerance" % prefix, type=float, default=DEFAULT_TOLERANCE,
                        help="an endpoint is hidden from a view when its depth exceeds the view's depth map by more than this share")


def settings_from_args(a, prefix="", views_per_batch=None):
    """The settings dict of the flags, or None when the edge length is not given (the stage is off)."""
    g = lambda k: getattr(a, prefix + k)
    if g("max_edge") is None:
        return None
    return {"max_edge": g("max_edge"), "rounds": g("rounds"), "depth_tolerance": getattr(a, prefix + "depth_tolerance", DEFAULT_TOLERANCE),
            "views_per_batch": views_per_batch}


def check_args(ap, a, prefix="", edge_flag=None):
    """The argument errors of the subdivision's settings, reported through ap.error."""
    s = settings_from_args(a, prefix)
    if s is None:
        return
    try:
        check_subdivide_settings(s)
    except ValueError as e:
        ap.error("%s: %s" % (edge_flag or "--%smax_edge" % prefix, e))


def summary_line(info):
    per = "; ".join("round %d: %d of %d edges seen, longest %.1f px, %d split -> %d vertices, %d faces"
                    % (i + 1, r["seen"], r["edges"], r["longest_px"], r["split"], r["vertices_out"], r["faces_out"])
                    for i, r in enumerate(info["rounds"]))
    return per + ("; stopped early" if info["stopped_early"] else "")


def main(argv=None):
    ap = argparse.ArgumentParser(description="subdivide a surface mesh (binary PLY) where predict's views outresolve it")
    ap.add_argument("--mesh", required=True, help="the mesh (a PLY mesh.write_ply wrote)")
    ap.add_argument("--mvs", required=True, help="predict's output folder: {name}_init.pfm, {name}_prob.pfm and {name}.txt")
    ap.add_argument("--out", required=True, help="the subdivided mesh (.ply)")
    ap.add_argument("--views_per_batch", type=int, default=None, help="views per call of the measure (default: all)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.max_edge is None:
        ap.error("--max_edge is required")
    try:
        s = check_subdivide_settings(settings_from_args(a, "", a.views_per_batch))
    except ValueError as e:
        ap.error(str(e))
    if not a.out.endswith(".ply"):
        ap.error("--out must end in .ply")
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is subdivided on the GPU (no CPU fallback)")
    from .mesh import load_mvs_views, read_ply, write_ply

    v, f = read_ply(a.mesh)
    views = load_mvs_views(a.mvs)
    info = {}
    out_v, out_f = subdivide(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), views, info=info, **s)
    write_ply(a.out, out_v, out_f)
    print("subdivided mesh %s: %d -> %d vertices, %d -> %d faces, %d views; %s" % (a.out, v.shape[0], out_v.shape[0], f.shape[0], out_f.shape[0],
                                                                                  len(views), summary_line(info)))
    return a.out


if __name__ == "__main__":
    main()
