"""The cloud's outlier removal (csrc/cloud_outliers.hip, deep3d_aerial_amd/cloud_outliers.py) on synthetic merged clouds: n points,
one per voxel column of a jittered surface as cloud.merge_points leaves them, 1 % of them floaters spread over the box; radius
= 3 voxels, k = 8.  Per n: device-event ms of d3d_cloud_keys, torch.sort, d3d_cloud_heads (timed for the record: the stage does not
call it, its searches run on the sorted point keys) and d3d_cloud_outliers_distances (the gather and the search + selection kernel
together: one warm-up, then --runs timed calls, each on its own events: median, min, max), the bytes the entry must move
(computed from the shapes) as a time at 8 TB/s and the share of the measured time that is, and the whole cloud_outliers.outlier_mask
call (its host reads included).  With --variant_library SO (a `make CLOUD_OUTLIERS=plain` build) the entry of both builds runs on
the same tensors, taking turns, and must give the same bits; plain_over_production is the ratio of the medians.  One torch
comparison at a size brute force can hold: torch.cdist + topk on --brute points, timed beside the whole outlier_mask, with the
share of points whose D agrees (cdist's arithmetic is not the rule's).  What bounds the kernel is not measured here: no kernel
trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/cloud_outliers_bench.py [--runs 5] [--points 1e6,1e7,1e8] [--brute 20000] [--variant_library SO]
        [--out profiles/cloud_outliers_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_common import PEAK_BYTES_PER_S, bind, stats, timed  # noqa: E402
from deep3d_aerial_amd import _geom, _lib, cloud, cloud_outliers  # noqa: E402

VOXEL = 0.1
RADIUS = 3 * VOXEL
K = 8


def make_cloud(n, seed=0):
    """(xyz, border): a side x side lattice of voxel columns with one point each, at a random place in its column on z = a smooth
    surface plus a jitter of a third of a voxel, and n / 100 floaters anywhere in the box; n = side^2 + floaters, shuffled."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    floaters = n // 100
    side = int(math.isqrt(n - floaters))
    floaters = n - side * side
    L = VOXEL * side
    u = torch.rand((side * side, 3), device="cuda", generator=gen)
    ij = torch.arange(side * side, device="cuda")
    x, y = ((ij % side) + u[:, 0]) * VOXEL, ((ij // side) + u[:, 1]) * VOXEL
    z = 2.0 + torch.sin(x * 0.7) * torch.cos(y * 0.5) + (u[:, 2] - 0.5) * (VOXEL / 1.5)
    f = torch.rand((floaters, 3), device="cuda", generator=gen) * torch.tensor([L, L, 4.0], device="cuda")
    xyz = torch.cat([torch.stack([x, y, z], 1), f]).float()
    xyz = xyz[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    return xyz, [-1.0, L + 1.0, -1.0, L + 1.0, 0.0, 4.0]


def run(n, runs, variant):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    xyz, border = make_cloud(n)
    g = cloud.CloudGrid(border, RADIUS)
    b = g.border
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    frac = torch.empty((n,), dtype=torch.int64, device="cuda")
    res = {"points": n, "grid": list(g.n), "radius": RADIUS, "k": K, "runs": runs}

    def keys_call():
        _lib.check(lib.d3d_cloud_keys(P(xyz), n, b[0], b[1], b[2], b[3], b[4], b[5], RADIUS, P(keys), P(frac), st), "d3d_cloud_keys")

    res["keys"] = stats(timed(keys_call, runs), 12 * n + 16 * n)
    del frac
    state = {}

    def sort_call():
        state["sorted"], state["order"] = torch.sort(keys)

    res["torch_sort"] = stats(timed(sort_call, runs))
    skeys, order = state["sorted"], state["order"]
    state.clear()
    del keys
    vox = torch.empty((n,), dtype=torch.int32, device="cuda")
    cells = torch.zeros((1,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_scratch_bytes, n, device="cuda")

    def heads_call():
        _lib.check(lib.d3d_cloud_heads(P(skeys), n, P(scratch), nbytes, P(vox), P(cells), st), "d3d_cloud_heads")

    res["heads_not_called_by_the_stage"] = stats(timed(heads_call, runs), 8 * n + 4 * n + 12 * n)
    res.update(cells=int(cells), points_per_cell=round(n / max(int(cells), 1), 3))
    del vox, scratch
    dist, nn = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
    sums = torch.zeros((3,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_outliers_scratch_bytes, n, device="cuda")

    def distances_call(L=lib, d=dist, c=nn, s=sums):
        _lib.check(L.d3d_cloud_outliers_distances(P(xyz), P(skeys), P(order), n, g.n[0], g.n[1], g.n[2], RADIUS, K, P(scratch), nbytes, P(d),
                                                  P(c), P(s), st), "d3d_cloud_outliers_distances")

    # gather: xyz and the order in, the float4 out; kernel: the keys, the float4 and the order in once (the candidates and the
    # searches re-read them from cache), D and nn out
    moved = n * (12 + 8 + 16) + n * (8 + 16 + 8 + 8)
    res["distances"] = stats(timed(distances_call, runs), moved)
    res["mean_neighbours"] = round(float(nn[nn >= 0].double().mean()), 3)
    if variant:
        other = bind(variant)
        dist2, nn2, sums2 = torch.empty_like(dist), torch.empty_like(nn), torch.zeros_like(sums)
        a_ms, b_ms = [], []
        for _ in range(runs):   # taking turns
            a_ms += timed(distances_call, 1)
            b_ms += timed(lambda: distances_call(other, dist2, nn2, sums2), 1)
        same = bool(torch.equal(dist, dist2) and torch.equal(nn, nn2) and torch.equal(sums, sums2))
        res["distances_variants"] = {"production": stats(a_ms, moved), "plain": stats(b_ms, moved), "variant_library": variant, "same_bits": same,
                                     "plain_over_production": round(float(np.median(b_ms)) / float(np.median(a_ms)), 3)}
        del dist2, nn2, sums2
    del skeys, order, dist, nn, scratch
    torch.cuda.empty_cache()
    # ---- the whole operator, host reads included
    res["outlier_mask"] = stats(timed(lambda: state.update(r=cloud_outliers.outlier_mask(xyz, border, RADIUS, K, 2.0, 0)), runs))
    res["outlier_mask"]["info"] = state["r"][1]
    res["bound"] = "unconfirmed (no kernel trace or counters in this run)"
    return res


def brute(n, runs):
    """torch.cdist + topk beside outlier_mask on n points."""
    xyz, border = make_cloud(n)
    state = {}

    def torch_call():
        d = torch.cdist(xyz.double(), xyz.double())
        d.fill_diagonal_(math.inf)
        near = d.topk(K, dim=1, largest=False).values
        e = torch.where(near < RADIUS, torch.round(near / RADIUS * 1024.0).clamp(max=1024.0), torch.full_like(near, 1024.0))
        state["D"] = e.sum(1).int()

    t_ms = timed(torch_call, runs)
    h_ms = timed(lambda: state.update(r=cloud_outliers.outlier_mask(xyz, border, RADIUS, K, 2.0, 0)), runs)
    dist = cloud_outliers.point_distances(xyz, cloud.CloudGrid(border, RADIUS), K)[0]
    return {"points": n, "torch_cdist_topk": stats(t_ms), "outlier_mask": stats(h_ms),
            "torch_over_hip": round(float(np.median(t_ms)) / float(np.median(h_ms)), 3),
            "share_of_points_with_equal_D": round(float((dist == state["D"]).double().mean()), 6)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1e6,1e7,1e8")
    ap.add_argument("--brute", type=int, default=20000, help="the size of the torch.cdist + topk comparison (0: skip it)")
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="a CLOUD_OUTLIERS=plain build of the library whose search + selection is timed beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_outliers_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/cloud_outliers_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "runs": []}
    for n in [int(float(x)) for x in a.points.split(",")]:
        res["runs"].append(run(n, a.runs, a.variant_library))
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
