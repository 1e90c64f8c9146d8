"""Flipping the mesh edges whose flip removes a cap triangle (csrc/mesh_flip.hip), off by default.

The marching-tetrahedra extraction emits slivers of two kinds.  A needle has one short edge, and the collapse (§4.24) removes it.
A cap has one obtuse angle near 180 degrees and no short edge, so no collapse touches it: only a flip of its long edge removes it.
Caps get near-zero projected area in the texture's view choice and degenerate normals in the refinement's sweep, and they are the
faces a later collapse most often refuses.  This stage swaps an interior manifold edge for the other diagonal of its two triangles
whenever that raises the worse of the two shape qualities, under a planarity guard, in rounds of independent flips.  Vertices never
move, the vertex and face counts never change, and the boundary never changes.  The rule is this project's own; it
does not claim to match OpenMVS's bRemoveSpikes (VCG's RemoveTVertexByFlip with its cap ratio 20).  All arithmetic is fp64 without
contraction; every dot product and squared length is summed left to right, (x x + y y) + z z.  There are no float atomics.

1. Input.  vertices [n,3] fp32 and faces [m,3] int32, every face with three distinct indices in 0 .. n - 1 (anything else is
   refused, as decimation and collapse refuse it).  max_angle is in degrees, in (0, 90], and has no default: the largest angle
   between the normals of the two triangles of a flipped edge.  rounds is 1 .. 64; its default, 16, is a setting, not a measurement,
   and so is max_angle.
2. Edges.  The undirected edges a < b of the mesh, numbered e = 0, 1, .. in (a, b) lexicographic order, as
   d3d_mesh_decimate_edges numbers them (subdivide.edge_list's list).
3. The pair.  The faces of a's row of the vertex -> face incidence that hold b.  The edge is a candidate only if there are exactly
   two, one holding the directed edge a->b (f_ab; its third corner is c) and the other b->a (f_ba; its third corner is d), and
   c != d.  Boundary edges, non-manifold edges and inconsistently oriented pairs are left alone.
4. Validity.  With N(v) the neighbours of v and x_v the fp64 position of v, all four must hold:
   (1) d is not in N(c): the new edge does not exist yet;
   (2) |N(a)| > 3 and |N(b)| > 3: each end loses a neighbour;
   (3) the planarity guard: with n1 = (x_b - x_a) x (x_c - x_a) and n2 = (x_a - x_b) x (x_d - x_b), the corner roles fixed by the
       edge and not by how the faces store their corners, n1.n2 >= 0 and (n1.n2)^2 >= cos^2(max_angle) (|n1|^2 |n2|^2); cos^2 is
       computed once on the host in fp64; a NaN fails;
   (4) no face turns over: the new faces are (a, d, c) and (b, c, d), and their normals (x_d - x_a) x (x_c - x_a) and
       (x_c - x_b) x (x_d - x_b) each have a dot product > 0 with n1 + n2.
5. Gain.  The quality of a triangle is Q = |n|^2 / S^2: with p0, p1, p2 its corners in increasing index order,
   n = (p1 - p0) x (p2 - p0) and S = (|p1 - p0|^2 + |p2 - p1|^2) + |p0 - p2|^2; Q = 0 when S = 0.  Q is a function of the vertex
   set alone, whatever rotation the face is stored in (1 / 12 for an equilateral triangle, 0 for one without area).  With
   min(x, y) = x when x < y, else y, the edge is a candidate only when min(Q(adc), Q(bcd)) > min(Q(abc), Q(bad)), strictly.
   Every flip then increases the ascending-sorted vector of all face qualities lexicographically, so the stage comes to rest.
6. Key.  key = (bits(fp32(min(Q(abc), Q(bad)))) << 32) | (e * 2654435761 mod 2^32): the worst pair first, the hash breaking ties.
   key = -1 where the edge is no candidate or lies past the edge count.  opp [E,4] int32 is (c, d, f_ab, f_ba), and 0 wherever
   the key is -1.
7. Winners.  A candidate claims a, b, c and d with the 64-bit minimum of the keys and wins when it reads its own key back on all
   four.  Winners share no vertex, hence no face, so tests (1) and (2), judged on the round's input, hold for all of them at
   once.  The claim is narrower than the decimation's (a, b and all their neighbours) on purpose: more flips per round.
8. Output.  A copy of the faces in which slot f_ab is (a, d, c) and slot f_ba is (b, c, d) for every winner.  Every other face
   and every vertex is untouched; there is no compaction.
9. Rounds.  The step repeats on its result with a fresh adjacency, incidence and edge list, up to `rounds` times, and stops early
   when a round has no winner.  That costs one device-to-host read of the counts per round.  With no winner at all the input
   tensors come back as they are.
The result is a function of the input arrays: the same bits run to run, whatever order the atomics land in.  Permuting the face
list gives the same set of faces, and so does rotating the corners of any input face: the pair is found by the cyclic order of the
corners, the normals take their corners from the edge, and Q from the sorted indices.  There is no CPU fallback.

    python -m deep3d_aerial_amd.flip --mesh IN.ply --out OUT.ply --max_angle DEG [--rounds R]
"""
import argparse
import ctypes
import math

import torch

from . import _lib
from ._geom import ptr as _ptr, stream as _stream
from .mesh import _decimate_arrays

DEFAULT_ROUNDS = 16   # a setting, not a measurement
MAX_ROUNDS = 64
_KEYS = ("max_angle", "rounds")


def check_flip_settings(settings):
    """The settings dict checked and completed: {"max_angle", "rounds"}.  max_angle has no default."""
    unknown = set(settings) - set(_KEYS)
    if unknown:
        raise ValueError("flip: unknown settings %s" % sorted(unknown))
    if settings.get("max_angle") is None:
        raise ValueError("flip needs max_angle (the largest angle between the two triangles of a flipped edge, in (0, 90] degrees)")
    try:
        max_angle = float(settings["max_angle"])
    except (TypeError, ValueError):
        max_angle = float("nan")
    if not 0 < max_angle <= 90:
        raise ValueError("flip max_angle %r must be an angle in (0, 90] degrees" % (settings["max_angle"],))
    rounds = DEFAULT_ROUNDS if settings.get("rounds") is None else settings["rounds"]
    try:
        whole = int(rounds) == rounds
    except (TypeError, ValueError):
        whole = False
    if not whole or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError("flip rounds %r must be an integer in 1 .. %d" % (rounds, MAX_ROUNDS))
    return {"max_angle": max_angle, "rounds": int(rounds)}


def cos2(max_angle):
    """cos^2 of max_angle degrees in fp64, as rule 4 (3) takes it."""
    c = math.cos(math.radians(float(max_angle)))
    return c * c


def topology(faces, n_vertices):
    """What a round reads of the connectivity, on the device: collapse.topology's dict ("offset", "nbr", "fixed", "face_offset",
    "face_index", "edges", "n_edges", "counts": [0] gets the winners)."""
    from .collapse import topology as _topology

    return _topology(faces, n_vertices)


def candidates(vertices, faces, csr, incidence, edges, n_edges, max_angle):
    """Rules 3-6 on the device: (key [E] int64, opp [E,4] int32) of the edges [E,2] (n_edges of them; subdivide.edge_list).  csr:
    mesh.adjacency's (offset, nbr, fixed); incidence: mesh.face_incidence's (face_offset, face_index).  No read."""
    s = check_flip_settings({"max_angle": max_angle})
    n, m, emax = int(vertices.shape[0]), int(faces.shape[0]), int(edges.shape[0])
    dev = vertices.device
    offset, nbr = csr[0], csr[1]
    foff, finc = incidence
    key = torch.empty((max(emax, 1),), dtype=torch.int64, device=dev)
    opp = torch.empty((max(emax, 1), 4), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().d3d_mesh_flip_candidates(_ptr(vertices), n, _ptr(faces), m, _ptr(offset), _ptr(nbr), _ptr(foff), _ptr(finc),
                                                    _ptr(edges), _ptr(n_edges), emax, cos2(s["max_angle"]), _ptr(key), _ptr(opp), _stream()),
               "d3d_mesh_flip_candidates")
    return key[:emax], opp[:emax]


def claim_apply(faces, topo, key, opp):
    """Rules 7 and 8: (out_faces [m,3] int32: the copy with the winners' slots rewritten, win [E] uint8, claim [n] int64);
    topo["counts"][0] gets the winners."""
    lib = _lib.load()
    n, m, emax = int(topo["offset"].shape[0]) - 1, int(faces.shape[0]), int(topo["edges"].shape[0])
    dev = faces.device
    st = _stream()
    edges, n_edges = topo["edges"], topo["n_edges"]
    n_win = ctypes.c_void_p(topo["counts"].data_ptr())
    claim = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    _lib.check(lib.d3d_mesh_flip_claim(n, _ptr(edges), _ptr(key), _ptr(opp), _ptr(n_edges), emax, _ptr(claim), n_win, st), "d3d_mesh_flip_claim")
    out_faces = torch.empty_like(faces)
    win = torch.empty((max(emax, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.d3d_mesh_flip_apply(_ptr(faces), m, _ptr(edges), _ptr(key), _ptr(opp), _ptr(n_edges), emax, _ptr(claim), _ptr(out_faces),
                                       _ptr(win), n_win, st), "d3d_mesh_flip_apply")
    return out_faces, win[:emax], claim[:n]


def _record(edges=0, candidates=0, winners=0):
    return {"edges": edges, "candidates": candidates, "winners": winners}


def _round(vertices, faces, n, m, s, detail=None):
    """flip_round on arrays and settings already checked."""
    if n == 0 or m == 0:
        return vertices, faces, _record()
    topo = topology(faces, n)
    edges = topo["edges"]
    key, opp = candidates(vertices, faces, (topo["offset"], topo["nbr"], topo["fixed"]), (topo["face_offset"], topo["face_index"]), edges,
                          topo["n_edges"], s["max_angle"])
    out_faces, win, claim = claim_apply(faces, topo, key, opp)
    valid = (key >= 0).sum().reshape(1)
    ne, nw, n_valid = torch.cat([topo["n_edges"], topo["counts"][:1], valid]).cpu().tolist()   # the round's one read
    if detail is not None:
        detail.update(offset=topo["offset"], nbr=topo["nbr"][:2 * ne], fixed=topo["fixed"], face_offset=topo["face_offset"],
                      face_index=topo["face_index"], edges=edges[:ne], n_edges=ne, key=key[:ne], opp=opp[:ne], claim=claim, win=win[:ne])
    if nw == 0:
        return vertices, faces, _record(ne, n_valid, 0)
    return vertices, out_faces, _record(ne, n_valid, nw)


def flip_round(vertices, faces, max_angle, detail=None):
    """One round (rules 2-8): (vertices, faces, record); with no winner the input tensors come back.  record: {"edges",
    "candidates", "winners"}.  detail (a dict) gets every pass's output: offset, nbr, fixed, face_offset, face_index, edges [E,2],
    n_edges, key [E] (-1: no candidate), opp [E,4], claim [n], win [E].  One device-to-host read after the checks of the input."""
    s = check_flip_settings({"max_angle": max_angle})
    vertices, faces, n, m = _decimate_arrays(vertices, faces, "flip")
    return _round(vertices, faces, n, m, s, detail)


def flip_edges(vertices, faces, max_angle, rounds=DEFAULT_ROUNDS, info=None):
    """The mesh with every edge flipped whose flip raises the worse quality of its two triangles, over up to `rounds` rounds, on the
    device: (vertices, faces); the vertices are the input's.  With nothing to flip the input tensors come back as they are.  info
    (a dict) gets {"edges", "candidates", "winners": one number per round, "rounds": the rounds run, "hit_max_rounds": the last
    allowed round still had a winner, "faces": m, "flips": the winners of all rounds}."""
    s = check_flip_settings({"max_angle": max_angle, "rounds": rounds})
    v, f, n, m = _decimate_arrays(vertices, faces, "flip")
    rec = {"edges": [], "candidates": [], "winners": [], "rounds": 0, "hit_max_rounds": False, "faces": m}
    won = False
    for k in range(s["rounds"] if n and m else 0):
        v, f, r = _round(v, f, n, m, s)
        rec["rounds"] += 1
        for key in ("edges", "candidates", "winners"):
            rec[key].append(r[key])
        if r["winners"] == 0:
            break
        won = True
        rec["hit_max_rounds"] = k + 1 == s["rounds"]
    rec["flips"] = sum(rec["winners"])
    if info is not None:
        info.update(rec)
    if not won:
        return vertices, faces
    return v, f


# ----------------------------------------------------------------------------------------
# settings and command line
# ----------------------------------------------------------------------------------------
def add_arguments(ap, prefix="", angle_flag=None):
    """The flip's settings as flags.  The angle is --<prefix>max_angle unless angle_flag names it (the mesh stage's --flip,
    predict's --mesh_flip)."""
    ap.add_argument(angle_flag or "--%smax_angle" % prefix, type=float, default=None, metavar="DEG", dest=prefix + "max_angle",
                    help="flip the mesh edges whose flip removes a cap triangle, where the two triangles meet at no more than DEG "
                         "degrees, in (0, 90]")
    ap.add_argument("--%srounds" % prefix, type=int, default=DEFAULT_ROUNDS, metavar="R",
                    help="flip rounds, each taking the independent flips (1 .. %d)" % MAX_ROUNDS)


def settings_from_args(a, prefix=""):
    """The settings dict of the flags, or None when the angle is not given (the stage is off)."""
    g = lambda k: getattr(a, prefix + k)
    if g("max_angle") is None:
        return None
    return {"max_angle": g("max_angle"), "rounds": g("rounds")}


def check_args(ap, a, prefix="", angle_flag=None):
    """The argument errors of the flip's settings, reported through ap.error."""
    s = settings_from_args(a, prefix)
    if s is None:
        return
    try:
        check_flip_settings(s)
    except ValueError as e:
        ap.error("%s: %s" % (angle_flag or "--%smax_angle" % prefix, e))


def summary_line(info):
    per = "; ".join("round %d: %d of %d edges candidates, %d flipped" % (i + 1, info["candidates"][i], info["edges"][i], w)
                    for i, w in enumerate(info["winners"]))
    if not per:
        return per
    return per + "; %d flips in %d faces%s" % (info["flips"], info["faces"], "; reached the round limit" if info["hit_max_rounds"] else "")


def main(argv=None):
    ap = argparse.ArgumentParser(description="flip the edges of a surface mesh (binary PLY) whose flip removes a cap triangle")
    ap.add_argument("--mesh", required=True, help="the mesh (a PLY mesh.write_ply wrote)")
    ap.add_argument("--out", required=True, help="the flipped mesh (.ply)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    if a.max_angle is None:
        ap.error("--max_angle is required")
    try:
        s = check_flip_settings(settings_from_args(a))
    except ValueError as e:
        ap.error(str(e))
    if not a.out.endswith(".ply"):
        ap.error("--out must end in .ply")
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is flipped on the GPU (no CPU fallback)")
    from .mesh import read_ply, write_ply

    v, f = read_ply(a.mesh)
    info = {}
    out_v, out_f = flip_edges(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), info=info, **s)
    write_ply(a.out, out_v, out_f)
    print("flipped mesh %s: %d vertices, %d faces; %s" % (a.out, v.shape[0], f.shape[0], summary_line(info) or "nothing to flip"))
    return a.out


if __name__ == "__main__":
    main()
