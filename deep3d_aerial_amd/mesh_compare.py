"""Comparison of a surface mesh with a reference cloud on the GPU: the surface is sampled deterministically at a stated spacing,
the samples are compared with the reference by the capped search of cloud_compare, and the error is brought back
onto the faces.

A mesh's vertices say little about its surface: a decimated roof of two triangles has four vertices, and its completeness against
10 000 LiDAR returns on that roof is about 0.  Sampled at a spacing s, every point of the surface has a sample within 2s/3.  The
rule below is this project's own; it does not claim to match any tool.

* Inputs.  vertices [nv,3] fp32, faces [m,3] int32 on one GPU, and a spacing s, finite and > 0.
* Per face f with corners (A, B, C) in the face's own order; all arithmetic fp64, every operation rounded once (no fused
  multiply-add):
  - L2 = the largest of the three squared edge lengths, each (dx dx + dy dy) + dz dz.
  - n_f = 0 when a corner coordinate is not finite or L2 is not a finite number > 0.
  - Otherwise q = sqrt(L2) / s and n_f = 1 for q <= 1, else ceil(q).
  - An n_f above N_MAX = 32768 is set to N_MAX and the face counts as clipped (sample() refuses a mesh with a clipped face).
  - The face gets n_f^2 samples: the centroids of the n_f^2 congruent sub-triangles of its n_f-fold edge subdivision.
* Sample t (0 .. n^2 - 1) of a face with n = n_f:
  - row r = floor(sqrt(t)), an exact integer square root; c = t - r^2, in 0 .. 2r; k = c >> 1.
  - integer weights (p, q, w) that sum to 3n:
    c even (upright):  p = 3(n - r) - 2, q = 3k + 1, w = 3(r - k) + 1;
    c odd (inverted):  p = 3(n - r) - 1, q = 3k + 2, w = 3(r - k) - 1.
  - per axis x = ((p A_x + q B_x) + w C_x) / (3n) in fp64, then rounded to fp32.
* Order.  The samples are ordered by (face in input order, t).
* Outputs.  offsets [m+1] int32, the exclusive scan of n_f^2; xyz [S,3] fp32; face [S] int32.
* Properties.
  - In exact arithmetic every point of a face lies within 2s/3 of a sample of that face: a sub-triangle's longest edge is at most
    s, its medians are no longer than its longest edge, and a point of a triangle is no further from the centroid than the
    farthest corner, which is 2/3 of a median away.
  - For well-shaped faces much longer than s the density is between about 2.3 and 4 samples per s^2 (n^2 samples on an area of
    sqrt(3)/4 (n s)^2 for an equilateral face, of (n s)^2 / 4 for a right isosceles one).  It is higher for slivers, whose area is
    small for their longest edge, and for faces not much longer than s (ceil rounds n up, and a face shorter than s still gets one
    sample).  So the accuracy direction weights slivers and small faces more: a stated bias, not corrected here.
  - The multiset of samples does not depend on the order of the faces, so e and both histograms of a comparison do not either.
  - The multiset may change in the last bit under a rotation of a face's corners: nothing is claimed for that case.
* Face error.  From the e [S] of a comparison and face [S]: per face sum int64 and keyed int32 over its samples with e >= 0, and
  worst int32, their maximum, -1 for a face with no keyed sample.  Integer atomics only: the same bits for any order.
* compare().  sample(), cloud_compare.prepare of either cloud, cloud_compare.nearest in both directions, one host read of the two
  histograms, cloud_compare.stats: the samples take the place of the evaluated cloud.

Out of scope: the exact point-to-triangle distance for the completeness direction (a reference point is held against the nearest
sample, up to 2s/3 beside the nearest surface point); area weights to remove the density bias; sampling by normals or colour; a
shift of large coordinates before the fp32 rounding; a registration of its own (see --transform below).  Ground truth is not an
input of a reconstruction run: pipeline.predict_and_fuse and predict have no key or flag for this.

The sampling and the face error are HIP (csrc/mesh_sample.hip); the scan is geom_scan, the keys d3d_cloud_keys, the search
d3d_cloud_compare_nearest, the statistics cloud_compare.stats, each as it is.

    python -m deep3d_aerial_amd.mesh_compare --mesh M.ply --reference B.ply --border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax --max_dist H
        --threshold T[,T...] --spacing S [--transform T.txt] [--json R.json] [--out_samples S.ply] [--out_accuracy EA.ply]
        [--out_completeness EB.ply] [--out_mesh EM.ply]

--transform: a 4 x 4 transform as cloud_register writes it; the mesh's vertices go through cloud_register.apply before anything
else, and the --out_* files carry the moved coordinates.  The mesh has no registration of its own: register its samples
(--out_samples) with cloud_register, then pass the transform here.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import _geom, _lib, cloud, cloud_compare
from ._geom import ptr as _ptr, stream as _stream

N_MAX = 32768
MAX_SAMPLES = (1 << 31) - 1


def _spacing(spacing):
    if not _geom.is_real(spacing, above=0):
        raise ValueError("spacing must be finite and > 0 (got %r)" % (spacing,))
    return float(spacing)


def sample(vertices, faces, spacing, max_samples=MAX_SAMPLES):
    """vertices [nv,3] fp32, faces [m,3] int32 on one GPU, a spacing -> (xyz [S,3] fp32, face [S] int32, offsets [m+1] int32) of the
    module's docstring, device tensors.  The host reads the two totals once; a clipped face (n_f above 32768) and more than
    max_samples samples are a ValueError that names the spacing and the numbers, raised before xyz is allocated or a sample is
    emitted.  CPU tensors are refused."""
    s = _spacing(spacing)
    if not _geom.is_int(max_samples, 0, MAX_SAMPLES):
        raise ValueError("max_samples must be an integer in 0 .. 2^31 - 1 (got %r)" % (max_samples,))
    vertices, faces, n, m = _geom.mesh_arrays(vertices, faces, 1, "sampled")
    dev = vertices.device
    lib = _lib.load()
    counts = torch.empty((m,), dtype=torch.int32, device=dev)
    offsets = torch.empty((m + 1,), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    scratch, nbytes = _geom.scratch(lib.d3d_mesh_sample_scratch_bytes, m, device=dev)
    pv = _ptr(vertices) if n else None
    pf = _ptr(faces) if m else None
    _lib.check(lib.d3d_mesh_sample_count(pv, n, pf, m, s, _ptr(scratch), nbytes, _ptr(counts) if m else None, _ptr(offsets), _ptr(totals),
                                         _stream()), "d3d_mesh_sample_count")
    total, clipped = totals.tolist()   # the one read
    if clipped:
        raise ValueError("spacing %r: %d of %d faces are longer than %d spacings (they would get %d^2 samples each): sample with a "
                         "larger spacing" % (s, clipped, m, N_MAX, N_MAX))
    if total > max_samples:
        raise ValueError("spacing %r: the %d faces get %d samples, more than max_samples = %d: sample with a larger spacing"
                         % (s, m, total, max_samples))
    del counts, scratch
    xyz = torch.empty((total, 3), dtype=torch.float32, device=dev)
    face = torch.empty((total,), dtype=torch.int32, device=dev)
    _lib.check(lib.d3d_mesh_sample_emit(pv, n, pf, m, _ptr(offsets), total, _ptr(xyz) if total else None, _ptr(face) if total else None,
                                        _stream()), "d3d_mesh_sample_emit")
    return xyz, face, offsets


def face_error(e, face, n_faces):
    """e [S] int32 of a comparison and face [S] int32 of sample() on one GPU -> (sum [m] int64, keyed [m] int32, worst [m] int32)
    per face over its samples with e >= 0; worst = -1 for a face with none.  Device tensors; the host reads nothing."""
    if not (isinstance(e, torch.Tensor) and isinstance(face, torch.Tensor)):
        raise TypeError("e and face must be tensors")
    if e.dtype != torch.int32 or face.dtype != torch.int32 or e.dim() != 1 or face.shape != e.shape:
        raise ValueError("e and face must be [S] int32 (got %s %s, %s %s)" % (tuple(e.shape), e.dtype, tuple(face.shape), face.dtype))
    if not _geom.is_int(n_faces, 0, (1 << 31) - 1):
        raise ValueError("n_faces must be an integer in 0 .. 2^31 - 1 (got %r)" % (n_faces,))
    if e.device.type != "cuda" or face.device != e.device:
        raise RuntimeError("the face error is summed on the GPU (no CPU fallback); got %s and %s" % (e.device, face.device))
    e, face, S, m, dev = e.contiguous(), face.contiguous(), int(e.shape[0]), int(n_faces), e.device
    if S >= 1 << 31:
        raise ValueError("%d samples: at most 2^31 - 1" % S)
    total = torch.empty((m,), dtype=torch.int64, device=dev)
    keyed = torch.empty((m,), dtype=torch.int32, device=dev)
    worst = torch.empty((m,), dtype=torch.int32, device=dev)
    ps = (lambda t: _ptr(t) if S else None)
    pm = (lambda t: _ptr(t) if m else None)
    _lib.check(_lib.load().d3d_mesh_sample_face_error(ps(e), ps(face), S, m, pm(total), pm(keyed), pm(worst), _stream()),
               "d3d_mesh_sample_face_error")
    return total, keyed, worst


def compare(vertices, faces, reference_xyz, border, max_dist, thresholds, spacing):
    """(result, {"samples": (xyz, face, e, idx), "reference": (e, idx), "faces": (sum, keyed, worst)}): the dict of
    cloud_compare.stats() for the samples of the mesh against the reference [n,3] fp32 (all on one GPU), with one more key
    "mesh": {"faces", "sampled_faces", "samples", "spacing"}; per direction the device tensors of cloud_compare.nearest(), and
    the error per face.  The host reads the sampling's totals, then the two histograms and the number of sampled faces in one
    read."""
    taus = cloud_compare.check_thresholds(thresholds, cloud_compare.check_max_dist(max_dist))
    s = _spacing(spacing)
    try:
        grid = cloud.CloudGrid(border, max_dist)
    except ValueError as e:
        raise ValueError("compare grid (border, max_dist as the voxel): %s" % e)
    cloud.points(reference_xyz, "reference_xyz")
    if isinstance(vertices, torch.Tensor) and vertices.is_cuda:
        cloud.on_gpu(reference_xyz, "reference_xyz", "the mesh is compared")
    xyz, face, offsets = sample(vertices, faces, s)
    m = int(offsets.shape[0]) - 1
    pa, pb = cloud_compare.prepare(xyz, grid), cloud_compare.prepare(reference_xyz, grid)
    ea, ia, ha = cloud_compare.nearest(xyz, reference_xyz, grid, pa, pb)
    eb, ib, hb = cloud_compare.nearest(reference_xyz, xyz, grid, pb, pa)
    per_face = face_error(ea, face, m)
    sampled = (offsets[1:] > offsets[:-1]).sum().reshape(1)
    both = torch.cat([ha, hb, sampled]).tolist()   # the one read
    bins = cloud_compare.BINS
    result = cloud_compare.stats(both[:bins], both[bins:2 * bins], grid.voxel, [tau for tau, _ in taus],
                                 (int(xyz.shape[0]), int(reference_xyz.shape[0])))
    result["mesh"] = {"faces": m, "sampled_faces": int(both[2 * bins]), "samples": int(xyz.shape[0]), "spacing": s}
    return result, {"samples": (xyz, face, ea, ia), "reference": (eb, ib), "faces": per_face}


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_SAMPLE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("face", "<i4")])


def error_mesh_bytes(vertices, faces, sum, keyed):
    """The bytes of an error mesh: a binary little-endian PLY of vertices [n,3] fp32 and faces [m,3] int32 with red green blue
    uchar on the face element (MeshLab reads face colours): E = sum // keyed of the face's keyed samples coloured by
    cloud_compare.error_cloud_bytes' formula, red = min(255, E >> 1), green = min(255, (1024 - E) >> 1), blue = 0; a face with no
    keyed sample is grey (128, 128, 128).  Host arrays or tensors."""
    v, f, total, keyed = _geom.host(vertices), _geom.host(faces), _geom.host(sum), _geom.host(keyed)
    n, m = int(v.shape[0]), int(f.shape[0])
    if v.dtype != np.float32 or v.shape != (n, 3) or f.dtype != np.int32 or f.shape != (m, 3):
        raise ValueError("vertices must be [n,3] float32 and faces [m,3] int32 (got %s %s, %s %s)" % (v.shape, v.dtype, f.shape, f.dtype))
    if total.dtype != np.int64 or total.shape != (m,) or keyed.dtype != np.int32 or keyed.shape != (m,):
        raise ValueError("sum must be [m] int64 and keyed [m] int32 (got %s %s, %s %s)" % (total.shape, total.dtype, keyed.shape, keyed.dtype))
    if m and (keyed.min() < 0 or total.min() < 0 or (total > cloud_compare.CAP * keyed.astype(np.int64)).any()):
        raise ValueError("sum must lie in 0 .. 1024 keyed and keyed must be >= 0")
    has = keyed > 0
    E = total // np.maximum(keyed, 1).astype(np.int64)
    rec = np.empty((m,), _FACE_DTYPE)
    rec["n"] = 3
    rec["v"] = f
    rec["red"] = np.where(has, np.minimum(255, E >> 1), 128)
    rec["green"] = np.where(has, np.minimum(255, (cloud_compare.CAP - E) >> 1), 128)
    rec["blue"] = np.where(has, 0, 128)
    head = ["ply", "format binary_little_endian 1.0", "comment error mesh (deep3d_aerial_amd.mesh_compare)", "element vertex %d" % n,
            "property float x", "property float y", "property float z", "element face %d" % m, "property list uchar int vertex_indices",
            "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    return ("\n".join(head) + "\n").encode("ascii") + np.ascontiguousarray(v, "<f4").tobytes() + rec.tobytes()


def samples_bytes(xyz, face):
    """The bytes of the samples: a binary little-endian PLY with x y z float and face int per sample, in sample order."""
    xyz, face = _geom.host(xyz), _geom.host(face)
    n = int(xyz.shape[0])
    if xyz.dtype != np.float32 or xyz.shape != (n, 3) or face.dtype != np.int32 or face.shape != (n,):
        raise ValueError("xyz must be [n,3] float32 and face [n] int32 (got %s %s, %s %s)" % (xyz.shape, xyz.dtype, face.shape, face.dtype))
    rec = np.empty((n,), _SAMPLE_DTYPE)
    for k, a in enumerate("xyz"):
        rec[a] = xyz[:, k]
    rec["face"] = face
    return _geom.record_ply_bytes("mesh samples (deep3d_aerial_amd.mesh_compare)", rec)


# ----------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description="accuracy, completeness and F-score of a surface mesh against a reference cloud")
    ap.add_argument("--mesh", default=None, help="the evaluated mesh (.ply as mesh.write_ply writes it)")
    ap.add_argument("--reference", default=None, help="the reference cloud (.ply, binary little-endian)")
    ap.add_argument("--border", type=cloud.parse_border6, default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (world units)")
    ap.add_argument("--max_dist", type=float, default=None, help="the cap of the distances (world units); further points count the cap")
    ap.add_argument("--threshold", type=cloud_compare.parse_thresholds, default=None, help="T[,T...]: the distances under which a point counts")
    ap.add_argument("--spacing", type=float, default=None, help="the spacing of the samples on the surface (world units)")
    ap.add_argument("--json", default=None, help="write the result here too (.json)")
    ap.add_argument("--out_samples", default=None, help="the samples: x y z and their face (.ply)")
    ap.add_argument("--out_accuracy", default=None, help="the samples coloured by their distance to the reference (.ply)")
    ap.add_argument("--out_completeness", default=None, help="the reference coloured by its distance to the samples (.ply)")
    ap.add_argument("--out_mesh", default=None, help="the mesh with its faces coloured by their mean distance to the reference (.ply)")
    from . import cloud_register

    cloud_register.add_transform_argument(ap)
    a = ap.parse_args(argv)
    for flag in ("mesh", "reference", "border", "max_dist", "threshold", "spacing"):
        if getattr(a, flag) is None:
            ap.error("--%s is required" % flag)
    plys = ("out_samples", "out_accuracy", "out_completeness", "out_mesh")
    for flag in plys:
        if getattr(a, flag) is not None and not str(getattr(a, flag)).endswith(".ply"):
            ap.error("--%s must end in .ply" % flag)
    if a.json is not None and not str(a.json).endswith(".json"):
        ap.error("--json must end in .json")
    outs = [os.path.abspath(str(p)) for p in [a.json] + [getattr(a, flag) for flag in plys] if p is not None]
    if len(set(outs)) != len(outs):
        ap.error("two of --json, --out_samples, --out_accuracy, --out_completeness and --out_mesh name the same file")
    if set(outs) & {os.path.abspath(str(a.mesh)), os.path.abspath(str(a.reference))}:
        ap.error("an output would overwrite an input")
    cloud_register.check_transform_argument(ap, a.transform, {os.path.abspath(str(a.mesh)), os.path.abspath(str(a.reference))}, outs)
    try:
        cloud_compare.check_thresholds(a.threshold, cloud_compare.check_max_dist(a.max_dist))
        cloud.CloudGrid(a.border, a.max_dist)
        _spacing(a.spacing)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("the mesh is compared on the GPU (no CPU fallback)")
    from . import mesh

    v, f = mesh.read_ply(a.mesh)
    xb = cloud_compare.read_xyz_ply(a.reference)
    dv, df, db = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(xb).cuda()
    if a.transform is not None:   # the vertices move first; the samples and the error mesh carry the moved coordinates
        dv = cloud_register.apply(dv, cloud_register.read_transform(a.transform))
        v = dv.cpu().numpy()
    result, found = compare(dv, df, db, a.border, a.max_dist, a.threshold, a.spacing)
    line = json.dumps(result)
    xyz, face, ea, _ = found["samples"]
    if a.out_samples is not None:
        _geom.write_bytes(a.out_samples, samples_bytes(xyz, face))
    if a.out_accuracy is not None:
        _geom.write_bytes(a.out_accuracy, cloud_compare.error_cloud_bytes(xyz, ea))
    if a.out_completeness is not None:
        _geom.write_bytes(a.out_completeness, cloud_compare.error_cloud_bytes(xb, found["reference"][0]))
    if a.out_mesh is not None:
        _geom.write_bytes(a.out_mesh, error_mesh_bytes(v, f, found["faces"][0], found["faces"][1]))
    if a.json is not None:
        _geom.write_bytes(a.json, (line + "\n").encode("ascii"))
    print(line)
    return result


if __name__ == "__main__":
    main()
