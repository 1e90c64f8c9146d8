"""The comparison of two point clouds (csrc/cloud_compare.hip, deep3d_aerial_amd/cloud_compare.py) on synthetic clouds: two clouds of
n points each, jittered samples of one surface -- one point per voxel column, at a random place in its column, drawn separately for
either cloud --; max_dist = 3 voxels (a few point spacings).  Per n: device-event ms of d3d_cloud_keys and torch.sort on one cloud,
of d3d_cloud_compare_nearest in either direction (the gather of the targets and the search kernel together: one warm-up, then --runs
timed calls, each on its own events: median, min, max), the bytes the entry must move (computed from the shapes) as a time at 8 TB/s
and the share of the measured time that is, the whole cloud_compare.compare call (both clouds keyed and sorted, both directions,
its host read included), and, in the same run, the same search by d3d_cloud_outliers_distances with k = 8 on one of the clouds at
the same radius: the new kernel does a subset of that work per candidate (one minimum and an index instead of a sorted list of
eight), so nearest_over_outliers_per_query should not exceed 1.  One torch comparison at a size brute force can hold: torch.cdist +
min on --brute points per cloud, timed beside the whole compare, with the share of points whose e agrees (cdist's arithmetic is not
the rule's).  What bounds the kernel is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and
writes --out).

    python tools/cloud_compare_bench.py [--runs 5] [--points 1e6,1e7,1e8] [--brute 20000] [--out profiles/cloud_compare_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_common import PEAK_BYTES_PER_S, stats, timed  # noqa: E402  (cloud_normals_bench and cloud_register_bench take them from here)
from deep3d_aerial_amd import _geom, _lib, cloud, cloud_compare  # noqa: E402

VOXEL = 0.1
MAX_DIST = 3 * VOXEL
K = 8
THRESHOLDS = [0.5 * VOXEL, VOXEL, 2 * VOXEL]


def make_clouds(n, seed=0):
    """(cloud, reference, border): a side x side lattice of voxel columns, n = side^2 points per cloud, one in every column at a
    random place in it, on z = a smooth surface plus a jitter of a third of a voxel; either cloud drawn on its own and shuffled."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    side = int(math.isqrt(n))
    L = VOXEL * side
    out = []
    for _ in range(2):
        u = torch.rand((side * side, 3), device="cuda", generator=gen)
        ij = torch.arange(side * side, device="cuda")
        x, y = ((ij % side) + u[:, 0]) * VOXEL, ((ij // side) + u[:, 1]) * VOXEL
        z = 2.0 + torch.sin(x * 0.7) * torch.cos(y * 0.5) + (u[:, 2] - 0.5) * (VOXEL / 1.5)
        xyz = torch.stack([x, y, z], 1).float()
        out.append(xyz[torch.randperm(side * side, device="cuda", generator=gen)].contiguous())
        del u, ij, x, y, z, xyz
    return out[0], out[1], [-1.0, L + 1.0, -1.0, L + 1.0, 0.0, 4.0]


def run(n, runs):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    xa, xb, border = make_clouds(n)
    n = int(xa.shape[0])
    g = cloud.CloudGrid(border, MAX_DIST)
    b = g.border
    res = {"points_per_cloud": n, "grid": list(g.n), "max_dist": MAX_DIST, "runs": runs}
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    frac = torch.empty((n,), dtype=torch.int64, device="cuda")

    def keys_call():
        _lib.check(lib.d3d_cloud_keys(P(xa), n, b[0], b[1], b[2], b[3], b[4], b[5], MAX_DIST, P(keys), P(frac), st), "d3d_cloud_keys")

    res["keys_one_cloud"] = stats(timed(keys_call, runs), 12 * n + 16 * n)
    state = {}
    res["torch_sort_one_cloud"] = stats(timed(lambda: state.update(s=torch.sort(keys)), runs))
    state.clear()
    del keys, frac
    pa, pb = cloud_compare.prepare(xa, g), cloud_compare.prepare(xb, g)
    e, idx = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
    hist = torch.zeros((cloud_compare.BINS,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_compare_scratch_bytes, n, n, device="cuda")

    def nearest_call(q, pq, t, pt):
        _lib.check(lib.d3d_cloud_compare_nearest(P(q), P(pq[0]), P(pq[1]), n, P(t), P(pt[0]), P(pt[1]), n, g.n[0], g.n[1], g.n[2], MAX_DIST,
                                                 P(scratch), nbytes, P(e), P(idx), P(hist), st), "d3d_cloud_compare_nearest")

    # gather: the targets' xyz and order in, the 16-byte records out; kernel: the queries' keys, order and xyz and the targets' keys
    # and records in once (the candidates and the searches re-read them from cache), e and idx out, the histogram
    moved = n * (12 + 8 + 16) + n * (8 + 8 + 12 + 8) + n * (8 + 16) + 2 * 8 * cloud_compare.BINS
    res["nearest_cloud_to_reference"] = stats(timed(lambda: nearest_call(xa, pa, xb, pb), runs), moved)
    res["found_share"] = round(float((idx >= 0).double().mean()), 6)
    res["nearest_reference_to_cloud"] = stats(timed(lambda: nearest_call(xb, pb, xa, pa), runs), moved)
    # ---- the outliers' search on the cloud, at the same radius: the same candidates per query (and the query itself skipped)
    dist, nn = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
    sums = torch.zeros((3,), dtype=torch.int64, device="cuda")
    oscratch, onbytes = _geom.scratch(lib.d3d_cloud_outliers_scratch_bytes, n, device="cuda")

    def outliers_call():
        _lib.check(lib.d3d_cloud_outliers_distances(P(xa), P(pa[0]), P(pa[1]), n, g.n[0], g.n[1], g.n[2], MAX_DIST, K, P(oscratch), onbytes,
                                                    P(dist), P(nn), P(sums), st), "d3d_cloud_outliers_distances")

    a_ms, o_ms = [], []
    for _ in range(runs):   # taking turns
        a_ms += timed(lambda: nearest_call(xa, pa, xb, pb), 1)
        o_ms += timed(outliers_call, 1)
    res["outliers_k8_same_cloud"] = {"nearest": stats(a_ms), "outliers_distances": stats(o_ms),
                                     "mean_neighbours": round(float(nn[nn >= 0].double().mean()), 3),
                                     "nearest_over_outliers_per_query": round(float(np.median(a_ms)) / float(np.median(o_ms)), 3)}
    del dist, nn, sums, oscratch, scratch, e, idx, hist, pa, pb
    torch.cuda.empty_cache()
    # ---- the whole operator: both clouds keyed and sorted, both directions, the host read of the two histograms
    res["compare"] = stats(timed(lambda: state.update(r=cloud_compare.compare(xa, xb, border, MAX_DIST, THRESHOLDS)), runs))
    res["compare"]["result"] = state["r"][0]
    res["bound"] = "not measured (no kernel trace or counters in this run)"
    return res


def brute(n, runs):
    """torch.cdist + min beside compare on n points per cloud."""
    xa, xb, border = make_clouds(n)
    state = {}

    def torch_call():
        d = torch.cdist(xa.double(), xb.double())
        for name, near in (("ea", d.min(1).values), ("eb", d.min(0).values)):
            state[name] = torch.where(near < MAX_DIST, torch.round(near / MAX_DIST * 1024.0).clamp(max=1024.0),
                                      torch.full_like(near, 1024.0)).int()

    t_ms = timed(torch_call, runs)
    h_ms = timed(lambda: state.update(r=cloud_compare.compare(xa, xb, border, MAX_DIST, THRESHOLDS)), runs)
    found = state["r"][1]
    return {"points_per_cloud": int(xa.shape[0]), "torch_cdist_min": stats(t_ms), "compare": stats(h_ms),
            "torch_over_hip": round(float(np.median(t_ms)) / float(np.median(h_ms)), 3),
            "share_of_points_with_equal_e": round(float(torch.cat([found["cloud"][0] == state["ea"],
                                                                   found["reference"][0] == state["eb"]]).double().mean()), 6)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1e6,1e7,1e8")
    ap.add_argument("--brute", type=int, default=20000, help="the size of the torch.cdist + min comparison (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_compare_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/cloud_compare_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "runs": []}
    for n in [int(float(x)) for x in a.points.split(",")]:
        res["runs"].append(run(n, a.runs))
        print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    if a.brute > 0:
        res["brute_force"] = brute(a.brute, a.runs)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
