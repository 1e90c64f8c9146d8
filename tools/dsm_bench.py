"""The DSM kernels (csrc/dsm.hip) at the reference's CREATEDSM size: a 2900 x 2900 grid at 0.2 m (config.yaml), on a synthetic
terrain with box roofs and 1 % single-point spikes, at N = 8 M and 32 M points.  Device-event time per call of points_to_dsm for
Max and Robust_Max, and of one MovingAverage pass (radius 2); the bytes each call must move (from shapes) against the HBM peak
(8.0 TB/s); and the same-box comparator: the same Robust_Max selection written with torch.sort on 64-bit (cell << 32 | key)
keys -- it lives only in this tool.  Both paths are checked to give the same raster.  Prints one JSON line (and writes --out).

    python tools/dsm_bench.py [--iters 10] [--sizes 8,32] [--out profiles/dsm_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep3d_aerial_amd import dsm  # noqa: E402

HBM = 8.0e12


def terrain(n, grid, seed=0):
    """Rolling ground, 40 box roofs 8-25 m high, 1 % of the points 30 m spikes; generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    wx, wy = grid.width * grid.unit[0], grid.height * grid.unit[1]
    x = grid.x_min + torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * wx
    y = grid.y_max - torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * wy
    z = 720.0 + 10.0 * torch.sin(x / 37.0) * torch.cos(y / 53.0)
    rng = np.random.default_rng(seed)
    for _ in range(40):
        cx, cy = grid.x_min + rng.uniform(0, wx), grid.y_max - rng.uniform(0, wy)
        hx, hy, hz = rng.uniform(5, 30), rng.uniform(5, 30), rng.uniform(8, 25)
        inside = ((x - cx).abs() < hx) & ((y - cy).abs() < hy)
        z = torch.where(inside, z + hz, z)
    z = z + 0.05 * torch.randn(n, device="cuda", generator=g, dtype=torch.float64)
    z = torch.where(torch.rand(n, device="cuda", generator=g) < 0.01, z + 30.0, z)
    return torch.stack([x, y, z], 1).to(torch.float32).contiguous()


def timed_ms(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_sort_robust_max(xyz, grid, trim=0.1):
    """The comparator: cell index in fp64 as the kernels compute it, ordered uint32 keys, one torch.sort of (cell << 32 | key)."""
    x, y, z = xyz[:, 0].double(), xyz[:, 1].double(), xyz[:, 2]
    j = torch.floor((x - grid.x_min) / grid.unit[0])
    i = torch.floor((grid.y_max - y) / grid.unit[1])
    keep = torch.isfinite(xyz).all(1) & (j >= 0) & (j < grid.width) & (i >= 0) & (i < grid.height)
    keep &= (z.double() >= grid.z_min) & (z.double() <= grid.z_max)
    cell = (i * grid.width + j)[keep].long()
    u = z[keep].view(torch.int32).long() & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)
    s, _ = torch.sort((cell << 32) | (0xFFFFFFFF - key))   # by cell, key descending
    sc = s >> 32
    cells = grid.width * grid.height
    count = torch.bincount(sc, minlength=cells)
    start = torch.cumsum(count, 0) - count
    t = torch.floor(trim * count.double()).long()
    full = count > 0
    k = 0xFFFFFFFF - (s[(start + t)[full]] & 0xFFFFFFFF)
    bits = torch.where(k >= 0x80000000, k & 0x7FFFFFFF, k ^ 0xFFFFFFFF)
    h = torch.full((cells,), float("nan"), dtype=torch.float32, device=xyz.device)
    h[full] = bits.to(torch.int32).view(torch.float32)
    return h.view(grid.shape), count.view(grid.shape)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", default="8,32", help="millions of points")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dsm_bench needs the GPU (no CPU timing is reported)")
    grid = dsm.DsmGrid([-430.0, 150.0, -330.0, 250.0, 700.0, 900.0], [0.2, 0.2])
    cells = grid.width * grid.height
    res = {"tool": "dsm_bench", "grid": [grid.width, grid.height], "unit": list(grid.unit), "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "hbm_peak_TB_s": HBM / 1e12}
    h0 = None
    for m in [int(s) for s in a.sizes.split(",")]:
        n = m * 1000 * 1000
        xyz = terrain(n, grid)
        r = {}
        # bytes each call must move (shapes): points read once per pass that reads them, rasters written / read once
        need = {"Max": 12 * n + cells * (4 + 4 + 4) + cells * (4 + 4 + 4),
                "Robust_Max": 12 * n + 4 * n + cells * 4 + cells * 4 * 4 + (12 + 4 + 4) * n + 4 * n + cells * (4 + 4 + 4) + 4 * n}
        for select in ("Max", "Robust_Max"):
            ms = timed_ms(lambda: dsm.points_to_dsm(xyz, grid, select), a.iters)
            r[select] = {"ms": round(ms, 3), "bytes": need[select], "TB_s": round(need[select] / ms / 1e9, 3),
                         "share_of_hbm": round(need[select] / ms / 1e9 / (HBM / 1e12), 3)}
        h, c = dsm.points_to_dsm(xyz, grid, "Robust_Max")
        ms = timed_ms(lambda: torch_sort_robust_max(xyz, grid), a.iters)
        th, tc = torch_sort_robust_max(xyz, grid)
        same = bool(torch.equal(tc.to(torch.int32), c) and torch.equal(th.view(torch.int32), h.view(torch.int32)))
        r["torch_sort_Robust_Max"] = {"ms": round(ms, 3), "same_raster": same}
        r["Robust_Max_speedup_vs_torch_sort"] = round(ms / r["Robust_Max"]["ms"], 2)
        r["filled_cells"] = int(torch.isfinite(h).sum())
        r["max_points_per_cell"] = int(c.max())
        h0 = h
        del xyz, th, tc
        res["N_%dM" % m] = r
    fill_bytes = cells * 4 * 2
    ms = timed_ms(lambda: dsm.fill_moving_average(h0, 2), a.iters)
    holes = torch.isnan(h0)
    res["MovingAverage_r2"] = {"ms": round(ms, 3), "bytes": fill_bytes, "TB_s": round(fill_bytes / ms / 1e9, 3),
                               "empty_cells": int(holes.sum())}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
