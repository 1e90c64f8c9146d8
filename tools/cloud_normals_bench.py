"""The normals of a point cloud (csrc/cloud_normals.hip) and the point-to-plane sums of the registration
(csrc/cloud_register.hip) on the synthetic clouds of tools/cloud_compare_bench.py; the radius and the cap are 3 voxels.
Per n, device-event ms (one warm-up, then --runs timed calls, the two sides of a comparison alternating):
  d3d_cloud_normals beside d3d_cloud_outliers_distances (k = 8) on the same cloud, the same keys and the same order: the same
    walk, so the difference is the arithmetic per neighbour (three divisions and ten integer sums against a sorted insertion) and
    the eigen-solve per point; both also as ns per query;
  d3d_cloud_register_plane_sums beside d3d_cloud_register_sums on the e and idx of one search, the normals being the estimated
    ones: the same streams plus 12 bytes of normal per counted pair.
At --torch points: the normals by torch (cdist, mask, einsum over all pairs in row blocks, torch.linalg.eigh) and the plane system
by torch (gather, float64 einsum: not the exact integers) beside the kernels.
What bounds a kernel is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/cloud_normals_bench.py [--runs 5] [--points 1e6,1e7,1e8] [--torch 2e4] [--out profiles/cloud_normals_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cloud_compare_bench as B  # noqa: E402
from deep3d_aerial_amd import _geom, _lib, cloud, cloud_compare, cloud_normals  # noqa: E402

RADIUS = B.MAX_DIST


def alternating(calls, runs):
    """{name: [ms]} of the calls timed in turn, runs rounds after one warm-up round."""
    ms = {name: [] for name in calls}
    for name, call in calls.items():
        call()
    torch.cuda.synchronize()
    for _ in range(runs):
        for name, call in calls.items():
            ms[name] += B.timed(call, 1)[-1:]
    return ms


def torch_normals(x, h, rows=4096):
    """Normals by torch over all pairs: the same rule in float64, no kernel of this project."""
    xd = x.double()
    out = []
    for k in range(0, len(xd), rows):
        a = xd[k:k + rows]
        near = (torch.cdist(a, xd) < h).double()
        delta = torch.round((xd[None, :, :] - a[:, None, :]) / h * 1024.0)
        kk = near.sum(1)
        s1 = torch.einsum("ij,ijr->ir", near, delta)
        s2 = torch.einsum("ij,ijr,ijc->irc", near, delta, delta)
        C = s2 - s1[:, :, None] * s1[:, None, :] / kk[:, None, None]
        out.append(torch.linalg.eigh(C)[1][:, :, 0])
    return torch.cat(out)


def torch_plane(moved, e, idx, ref, nrm, g):
    """H and v of the plane step by torch in float64 (not the exact integers)."""
    ok = idx >= 0
    j = idx.clamp(min=0).long()
    o = torch.tensor(g.border[0::2], dtype=torch.float64, device=moved.device)
    c = o + 0.5 * g.voxel * torch.tensor(g.n, dtype=torch.float64, device=moved.device)
    a, b, m = moved.double(), ref.index_select(0, j).double(), nrm.index_select(0, j).double() * ok[:, None]
    G = torch.cat([torch.linalg.cross(a - c, m), m], 1)
    r = ((a - b) * m).sum(1)
    return torch.einsum("ni,nj->ij", G, G), torch.einsum("ni,n->i", G, r)


def run(n, runs, with_torch):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    xa, xb, border = B.make_clouds(n)
    n = int(xb.shape[0])
    g = cloud.CloudGrid(border, RADIUS)
    res = {"points_per_cloud": n, "grid": list(g.n), "radius": RADIUS, "runs": runs}
    skeys, order = cloud.sorted_keys(xb, g)
    normals = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    count = torch.empty((n,), dtype=torch.int32, device="cuda")
    flat = torch.empty((n,), dtype=torch.int32, device="cuda")
    dist = torch.empty((n,), dtype=torch.int32, device="cuda")
    osums = torch.zeros((3,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_normals_scratch_bytes, n, device="cuda")

    def normals_call():
        _lib.check(lib.d3d_cloud_normals(P(xb), P(skeys), P(order), n, g.n[0], g.n[1], g.n[2], RADIUS, 0, P(scratch), nbytes, P(normals),
                                         P(count), P(flat), None, st), "d3d_cloud_normals")

    def outliers_call():
        _lib.check(lib.d3d_cloud_outliers_distances(P(xb), P(skeys), P(order), n, g.n[0], g.n[1], g.n[2], RADIUS, 8, P(scratch), nbytes, P(dist),
                                                    P(flat), P(osums), st), "d3d_cloud_outliers_distances")

    ms = alternating({"outliers": outliers_call, "normals": normals_call}, runs)
    normals_call()   # (flat was the outliers' nn in between)
    for name in ms:
        res[name] = dict(B.stats(ms[name]), ns_per_query=round(float(np.median(ms[name])) * 1e6 / n, 3))
    res["normals_over_outliers"] = round(res["normals"]["ms_median"] / res["outliers"]["ms_median"], 3)
    res["mean_neighbours"] = round(float(count.double().mean()), 2)
    res["points_with_a_normal"] = int((flat >= 0).sum())
    if with_torch:
        t_ms = B.timed(lambda: torch_normals(xb, RADIUS), runs)
        tn = torch_normals(xb, RADIUS)
        has = flat >= 0
        cosine = (tn[has] * normals[has].double()).sum(1).abs()
        res["torch_normals"] = dict(B.stats(t_ms), torch_over_hip=round(float(np.median(t_ms)) / res["normals"]["ms_median"], 1),
                                    smallest_abs_cosine_to_the_kernel=float(cosine.min()))
        del tn
    del skeys, order, count, flat, dist, scratch
    pb = cloud_compare.prepare(xb, g)
    e, idx, _ = cloud_compare.nearest(xa, xb, g, None, pb)
    del pb
    b = g.border
    sums27 = torch.empty((27,), dtype=torch.int64, device="cuda")
    sums87 = torch.empty((87,), dtype=torch.int64, device="cuda")

    def point_call():
        _lib.check(lib.d3d_cloud_register_sums(P(xa), P(e), P(idx), n, P(xb), n, b[0], b[2], b[4], RADIUS, 1024, P(sums27), st),
                   "d3d_cloud_register_sums")

    def plane_call():
        _lib.check(lib.d3d_cloud_register_plane_sums(P(xa), P(e), P(idx), n, P(xb), P(normals), n, g.n[0], g.n[1], g.n[2], b[0], b[2], b[4],
                                                     RADIUS, 1024, P(sums87), st), "d3d_cloud_register_plane_sums")

    ms = alternating({"point_sums": point_call, "plane_sums": plane_call}, runs)
    counted = int(sums87[0])
    res["point_sums"] = dict(B.stats(ms["point_sums"], 20 * n + 12 * int(sums27[0])), counted_pairs=int(sums27[0]))
    res["plane_sums"] = dict(B.stats(ms["plane_sums"], 20 * n + 24 * counted), counted_pairs=counted)
    res["plane_over_point"] = round(res["plane_sums"]["ms_median"] / res["point_sums"]["ms_median"], 3)
    if with_torch:
        t_ms = B.timed(lambda: torch_plane(xa, e, idx, xb, normals, g), runs)
        res["torch_plane"] = dict(B.stats(t_ms), torch_over_hip=round(float(np.median(t_ms)) / res["plane_sums"]["ms_median"], 1))
    res["bound"] = "not measured (no kernel trace or counters in this run)"
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1e6,1e7,1e8")
    ap.add_argument("--torch", default="2e4", help="the size at which torch computes the same beside the kernels (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_normals_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/cloud_normals_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": B.PEAK_BYTES_PER_S, "runs": []}
    sizes = [int(float(x)) for x in a.points.split(",")]
    t = int(float(a.torch))
    for n in ([t] if t and t not in sizes else []) + sizes:
        res["runs"].append(run(n, a.runs, n == t))
        print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
