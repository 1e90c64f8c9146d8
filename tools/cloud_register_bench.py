"""The registration of a point cloud to a reference (csrc/cloud_register.hip, deep3d_aerial_amd/cloud_register.py) on the synthetic
clouds of tools/cloud_compare_bench.py: two jittered samples of one surface, n points each, drawn separately; the evaluated one
turned about the vertical through the middle so that its rim moves a voxel, and shifted by (0.05, -0.04, 0.03); the cap is 3 voxels.
Per n, device-event ms (one warm-up, then --runs timed calls, each on its own events: median, min, max) of
  d3d_cloud_transform, with the 24 n bytes it must move as a time at 8 TB/s and the share of the measured time that is;
  d3d_cloud_register_sums on the e and idx of the search, likewise at 20 n bytes of streams (xyz, e, idx) plus 12 bytes per counted
    pair for the gathered reference point (the least it can move: a gather fetches whole sectors);
  the parts of one iteration as cloud_register.register runs it: transform, keys, sort, nearest, sums, and the host's read of the 27
    sums (host clock around .tolist() on a finished tensor);
  one whole iteration (host clock, the solve included) and one whole registration with --iterations at most (host clock), with its
    iterations, its reasons and the corner error against the motion that was applied.
At --torch points: the same 27 integers by torch (index_select, int64 products, sum) beside the kernel, and whether they are equal.
What bounds a kernel is not measured here: no kernel trace and no counters are taken.  Not measured at all: real LiDAR, clouds of
unequal density, partial overlap.  Prints one JSON line (and writes --out).

    python tools/cloud_register_bench.py [--runs 5] [--points 1e6,1e7,1e8] [--torch 1e7] [--iterations 30]
        [--out profiles/cloud_register_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cloud_compare_bench as B  # noqa: E402
from deep3d_aerial_amd import _geom, _lib, cloud, cloud_compare, cloud_register  # noqa: E402

MAX_DIST = B.MAX_DIST
SHIFT = (0.05, -0.04, 0.03)


def motion(border):
    """The 4 x 4 motion of the evaluated cloud: a turn about the vertical through the border's middle that moves the rim by one
    voxel, then SHIFT."""
    cx, cy = 0.5 * (border[0] + border[1]), 0.5 * (border[2] + border[3])
    a = B.VOXEL / (0.5 * (border[1] - border[0]))
    M = np.eye(4)
    M[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    c = np.array([cx, cy, 0.0])
    M[:3, 3] = c - M[:3, :3] @ c + np.array(SHIFT)
    return M


def timed_host(call, runs):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def corner_error(T, truth, border):
    c = np.array([[border[i], border[2 + j], border[4 + k], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    d = (c @ T.T - c @ truth.T)[:, :3]
    return float(np.sqrt((d * d).sum(1)).max())


def torch_sums(moved, e, idx, ref, grid, e_max):
    """The 27 sums by torch: the same integers, no kernel of this project."""
    o = torch.tensor(grid.border[0::2], dtype=torch.float64, device=moved.device)
    h = torch.tensor(grid.voxel, dtype=torch.float64, device=moved.device)   # a tensor: torch divides by one, and multiplies by 1 / h for a number
    ok = (idx >= 0) & (e <= e_max)
    w = ok.long()[:, None]
    a = torch.round((moved.double() - o) / h * 1024.0).long() * w
    b = torch.round((ref.index_select(0, idx.clamp(min=0).long()).double() - o) / h * 1024.0).long() * w
    prod = a[:, :, None] * b[:, None, :]
    el = e.long() * ok.long()
    return torch.cat([ok.sum().reshape(1), a.sum(0), b.sum(0), (prod & 0xFFFFFFFF).sum(0).reshape(-1), (prod >> 32).sum(0).reshape(-1),
                      el.sum().reshape(1), (el * el).sum().reshape(1)])


def run(n, runs, iterations, with_torch):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    xa, xb, border = B.make_clouds(n)
    n = int(xa.shape[0])
    M = motion(border)
    xa = cloud_register.apply(xa, M)     # the evaluated cloud, moved
    g = cloud.CloudGrid(border, MAX_DIST)
    b = g.border
    res = {"points_per_cloud": n, "grid": list(g.n), "max_dist": MAX_DIST, "runs": runs}
    eye = torch.tensor(np.eye(4)[:3].reshape(-1).tolist(), dtype=torch.float64, device="cuda")
    moved = torch.empty((n, 3), dtype=torch.float32, device="cuda")

    def transform_call():
        _lib.check(lib.d3d_cloud_transform(P(xa), n, P(eye), P(moved), st), "d3d_cloud_transform")

    res["transform"] = B.stats(B.timed(transform_call, runs), 24 * n)
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    frac = torch.empty((n,), dtype=torch.int64, device="cuda")

    def keys_call():
        _lib.check(lib.d3d_cloud_keys(P(moved), n, b[0], b[1], b[2], b[3], b[4], b[5], MAX_DIST, P(keys), P(frac), st), "d3d_cloud_keys")

    res["keys"] = B.stats(B.timed(keys_call, runs))
    state = {}
    res["torch_sort"] = B.stats(B.timed(lambda: state.update(s=torch.sort(keys)), runs))
    state.clear()
    del keys, frac
    pa, pb = cloud_compare.prepare(moved, g), cloud_compare.prepare(xb, g)
    res["nearest"] = B.stats(B.timed(lambda: state.update(r=cloud_compare.nearest(moved, xb, g, pa, pb)), runs))
    e, idx, _ = state.pop("r")
    del pa
    sums = torch.empty((27,), dtype=torch.int64, device="cuda")

    def sums_call():
        _lib.check(lib.d3d_cloud_register_sums(P(moved), P(e), P(idx), n, P(xb), n, b[0], b[2], b[4], MAX_DIST, 1024, P(sums), st),
                   "d3d_cloud_register_sums")

    ms = B.timed(sums_call, runs)
    counted = int(sums[0])
    res["sums"] = B.stats(ms, 20 * n + 12 * counted + 27 * 8)
    res["sums"]["counted_pairs"] = counted
    res["host_read_of_the_sums"] = B.stats(timed_host(lambda: sums.tolist(), runs))
    if with_torch:
        t_ms = B.timed(lambda: state.update(t=torch_sums(moved, e, idx, xb, g, 1024)), runs)
        res["torch_sums"] = dict(B.stats(t_ms), torch_minus_kernel=(state.pop("t") - sums).tolist(),
                                 torch_over_hip=round(float(np.median(t_ms)) / float(np.median(ms)), 3))
        res["torch_sums"]["equal_to_the_kernel"] = not any(res["torch_sums"]["torch_minus_kernel"])
        torch.cuda.empty_cache()

    def iteration():
        m = cloud_register.apply(xa, np.eye(4))
        ee, ii, _ = cloud_compare.nearest(m, xb, g, None, pb)
        cloud_register.solve(cloud_register.pair_sums(m, ee, ii, xb, g).tolist(), g)

    res["iteration"] = B.stats(timed_host(iteration, runs))
    del moved, e, idx, pb
    torch.cuda.empty_cache()
    res["registration"] = B.stats(timed_host(lambda: state.update(r=cloud_register.register(xa, xb, border, [MAX_DIST], max_iterations=iterations)), runs))
    T, log, _ = state.pop("r")
    res["registration"].update(iterations=len(log), reasons=[x["reason"] for x in log if "reason" in x], first=log[0], last=log[-1],
                               corner_error_before=corner_error(np.eye(4), np.linalg.inv(M), border),
                               corner_error_after=corner_error(T, np.linalg.inv(M), border))
    parts = {k: res[k]["ms_median"] for k in ("transform", "keys", "torch_sort", "nearest", "sums", "host_read_of_the_sums")}
    res["largest_part_of_an_iteration"] = max(parts, key=parts.get)
    res["bound"] = "not measured (no kernel trace or counters in this run)"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1e6,1e7,1e8")
    ap.add_argument("--torch", default="1e7", help="the size at which torch computes the same sums beside the kernel (0: never)")
    ap.add_argument("--iterations", type=int, default=30, help="max_iterations of the whole registration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_register_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/cloud_register_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": B.PEAK_BYTES_PER_S, "runs": [],
           "unmeasured": ["real LiDAR", "clouds of unequal density", "partial overlap", "what bounds either kernel (no trace, no counters)"]}
    for n in [int(float(x)) for x in a.points.split(",")]:
        res["runs"].append(run(n, a.runs, a.iterations, n == int(float(a.torch))))
        print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
