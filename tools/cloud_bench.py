"""The point-cloud merge (csrc/cloud.hip cloud_*, deep3d_aerial_amd/cloud.py) on synthetic fused points: n points on a jittered
surface, about 5 to 10 to a voxel as the fused clouds of overlapping views have them, with unit normals and colours.  Per n:
device-event ms of every entry point on its own (keys, heads, accumulate, neighbours with min_points 4, finalize) and of
torch.sort between them (one warm-up, then --runs timed calls, each on its own events: median, min, max), the bytes each kernel
must move (computed from the shapes) as a time at 8 TB/s and the share of the measured time that is, and the whole
cloud.merge_points call (its two host reads included).  The yardstick is what a user writes without this stage, in the same
tool: after the same torch.sort, torch.unique_consecutive for the voxel of every point and index_add_ of int64 rows for the sums;
it is timed beside heads + accumulate, which it replaces, and must give the same integers.  With --variant_library SO (a
`make CLOUD=plain` build) the accumulation of both builds runs on the same tensors, taking turns, and must give the same bits.
What bounds the kernels is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/cloud_bench.py [--runs 5] [--points 1e6,1e7,1e8] [--variant_library SO] [--out profiles/cloud_bench.json]"""
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
from deep3d_aerial_amd import _geom, _lib, cloud  # noqa: E402

VOXEL = 0.1


def make_points(n, seed=0):
    """(xyz, normal, color, grid): n points over a square of side L = VOXEL sqrt(n / 10) on z = a smooth surface plus a jitter of
    a third of a voxel, all inside the grid."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    L = VOXEL * math.sqrt(n / 10.0)
    u = torch.rand((n, 3), device="cuda", generator=gen)
    x, y = u[:, 0] * L, u[:, 1] * L
    z = 2.0 + torch.sin(x * 0.7) * torch.cos(y * 0.5) + (u[:, 2] - 0.5) * (VOXEL / 1.5)
    xyz = torch.stack([x, y, z], 1).contiguous()
    nrm = torch.randn((n, 3), device="cuda", generator=gen)
    nrm = (nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-6)).contiguous()
    col = torch.randint(0, 256, (n, 3), device="cuda", generator=gen, dtype=torch.int32)
    grid = cloud.CloudGrid([-1.0, L + 1.0, -1.0, L + 1.0, 0.0, 4.0], VOXEL)
    return xyz, nrm, col, grid


def run(n, runs, variant):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    xyz, nrm, col, g = make_points(n)
    b, v = g.border, g.voxel
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    frac = torch.empty((n,), dtype=torch.int64, device="cuda")
    vox = torch.empty((n,), dtype=torch.int32, device="cuda")
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_cloud_scratch_bytes, n, device="cuda")
    scan = lambda m: 12 * m   # geom_scan: a pass that reads the values, one that reads them again and writes the sums
    res = {"points": n, "grid": list(g.n), "voxel": v, "runs": runs}

    def keys_call():
        _lib.check(lib.d3d_cloud_keys(P(xyz), n, b[0], b[1], b[2], b[3], b[4], b[5], v, P(keys), P(frac), st), "d3d_cloud_keys")

    res["keys"] = stats(timed(keys_call, runs), 12 * n + 16 * n)
    state = {}

    def sort_call():
        state["sorted"], state["order"] = torch.sort(keys)

    res["torch_sort"] = stats(timed(sort_call, runs))
    skeys, order = state["sorted"], state["order"]

    def heads_call():
        _lib.check(lib.d3d_cloud_heads(P(skeys), n, P(scratch), nbytes, P(vox), P(counts[0:1]), st), "d3d_cloud_heads")

    res["heads"] = stats(timed(heads_call, runs), 8 * n + 4 * n + scan(n))
    nv = int(counts[0])
    ukeys = torch.empty((nv,), dtype=torch.int64, device="cuda")
    count = torch.empty((nv,), dtype=torch.int32, device="cuda")
    acc = torch.empty((nv, 9), dtype=torch.int64, device="cuda")

    def accumulate_call(L=lib, a=acc, c=count):
        _lib.check(L.d3d_cloud_accumulate(P(skeys), P(order), P(vox), P(frac), P(nrm), P(col), n, nv, P(ukeys), P(c), P(a), st),
                   "d3d_cloud_accumulate")

    acc_bytes = n * (8 + 8 + 4 + 8 + 12 + 12) + nv * (8 + 2 * 4 + 2 * 72)   # the clear and the final values of count and acc
    res["accumulate"] = stats(timed(accumulate_call, runs), acc_bytes)
    res.update(voxels=nv, points_per_voxel=round(n / max(nv, 1), 3))
    if variant:
        other = bind(variant)
        acc2, count2 = torch.empty_like(acc), torch.empty_like(count)
        a_ms, b_ms = [], []
        for _ in range(runs):   # taking turns
            a_ms += timed(accumulate_call, 1)
            b_ms += timed(lambda: accumulate_call(other, acc2, count2), 1)
        res["accumulate_variants"] = {"production": stats(a_ms, acc_bytes), "variant": stats(b_ms, acc_bytes), "variant_library": variant,
                                      "same_bits": bool(torch.equal(acc, acc2) and torch.equal(count, count2))}
        del acc2, count2
    keep = torch.empty((nv,), dtype=torch.int32, device="cuda")
    pos = torch.empty((nv,), dtype=torch.int32, device="cuda")
    scratch2, nbytes2 = _geom.scratch(lib.d3d_cloud_scratch_bytes, nv, device="cuda")

    def neighbours_call():
        _lib.check(lib.d3d_cloud_neighbours(P(ukeys), P(count), nv, g.n[0], g.n[1], g.n[2], 4, P(scratch2), nbytes2, P(keep), P(pos),
                                            P(counts[1:2]), st), "d3d_cloud_neighbours")

    # the searches re-read the keys from cache; what must move is the keys and counts once, the flags, and two scans
    res["neighbours"] = stats(timed(neighbours_call, runs), nv * (8 + 4 + 4) + 2 * scan(nv))
    nk = int(counts[1])
    out = [torch.empty((nk, 3), dtype=torch.float32, device="cuda"), torch.empty((nk, 3), dtype=torch.float32, device="cuda"),
           torch.empty((nk, 3), dtype=torch.uint8, device="cuda"), torch.empty((nk,), dtype=torch.int32, device="cuda")]

    def finalize_call():
        _lib.check(lib.d3d_cloud_finalize(P(ukeys), P(count), P(acc), P(keep), P(pos), nv, nk, b[0], b[1], b[2], b[3], b[4], b[5], v,
                                          P(out[0]), P(out[1]), P(out[2]), P(out[3]), st), "d3d_cloud_finalize")

    res["finalize"] = stats(timed(finalize_call, runs), nv * (8 + 4 + 72 + 4 + 4) + nk * (12 + 12 + 3 + 4))
    res["kept_with_min_points_4"] = nk
    # ---- the yardstick: unique_consecutive + index_add_ in int64 on the same sorted keys
    state = {}

    def torch_call():
        uk, inv, cnt = torch.unique_consecutive(skeys, return_inverse=True, return_counts=True)
        f = frac[order]
        rows = torch.cat([torch.stack([f & 0xffff, (f >> 16) & 0xffff, f >> 32], 1),
                          torch.round(nrm[order].double() * 1048576.0).long(), col[order].clamp(0, 255).long()], 1)
        sums = torch.zeros((uk.shape[0], 9), dtype=torch.int64, device="cuda")
        sums.index_add_(0, inv, rows)
        state.update(uk=uk, cnt=cnt, sums=sums)

    tms = timed(torch_call, runs)
    hip = [res["heads"]["ms_median"] + res["accumulate"]["ms_median"]]
    same = bool(torch.equal(state["uk"], ukeys) and torch.equal(state["cnt"].int(), count) and torch.equal(state["sums"], acc))
    res["torch_unique_index_add"] = dict(stats(tms), same_integers=same, hip_heads_plus_accumulate_ms=round(hip[0], 4),
                                         torch_over_hip=round(float(np.median(tms)) / hip[0], 3) if hip[0] > 0 else None)
    state.clear()
    del keys, frac, vox, skeys, order, ukeys, count, acc, keep, pos, out
    torch.cuda.empty_cache()
    # ---- the whole operator, host reads included, and its result against the staged calls
    res["merge_points"] = stats(timed(lambda: state.update(c=cloud.merge_points(xyz, nrm, col, g, 4)), runs))
    res["merge_points"]["voxels_kept"] = int(state["c"]["count"].shape[0])
    res["bound"] = "unconfirmed (no kernel trace or counters in this run)"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--points", default="1e6,1e7,1e8")
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="a CLOUD=plain build of the library whose accumulation is timed beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/cloud_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "runs": []}
    for n in [int(float(x)) for x in a.points.split(",")]:
        res["runs"].append(run(n, a.runs, a.variant_library))
        print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
