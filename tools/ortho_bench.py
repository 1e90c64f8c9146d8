"""The orthophoto kernels (csrc/ortho.hip) at the DSM's size: a 2900 x 2900 grid at 0.2 m on a terrain DSM (rolling ground plus
boxes, 1 % empty cells; synthetic.make_ortho_scene) with V = 32 and V = 128 views of 2752 x 1856, half nadir, half oblique.
Device-event time per call of select_views and of colorize; the mean number of candidate views per cell (in the image and in
front of the view) and the share of them that pass the depth test; the bytes each call must move (from shapes and those counts)
against the HBM peak (8.0 TB/s); and the same-box comparator: the same selection in plain torch, one view at a time (projection,
gather, torch.minimum on the keys) -- it lives only in this tool.  Both paths are checked to give the same key raster.  Prints one
JSON line (and writes --out).

    python tools/ortho_bench.py [--iters 5] [--views 32,128] [--out profiles/ortho_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep3d_aerial_amd import ortho, synthetic as S  # noqa: E402

HBM = 8.0e12
EMPTY = (1 << 63) - 1


def timed_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_select(height, grid, views, tol=ortho.DEFAULT_TOLERANCE):
    """The comparator: ortho.py's semantics in fp64 torch, one view at a time.  Also returns the candidate counts per cell
    (projected into the image, in front) and how many of them pass the depth test."""
    H, W = grid.shape
    dev = height.device
    X0 = (grid.x_min + (torch.arange(W, dtype=torch.float64, device=dev) + 0.5) * grid.unit[0]).expand(H, W)
    X1 = (grid.y_max - (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) * grid.unit[1])[:, None].expand(H, W)
    live = torch.isfinite(height)
    X2 = torch.where(live, height, torch.zeros_like(height)).double()
    key = torch.full((H, W), EMPTY, dtype=torch.int64, device=dev)
    n_cand = torch.zeros((H, W), dtype=torch.int32, device=dev)
    n_pass = torch.zeros((H, W), dtype=torch.int32, device=dev)
    for v in views:
        R, t, K, C = v.R.tolist(), v.t.tolist(), v.K.tolist(), v.C.tolist()
        p = [R[r][0] * X0 + R[r][1] * X1 + R[r][2] * X2 + t[r] for r in range(3)]
        q = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
        u, w = q[0] / q[2], q[1] / q[2]
        ok = live & (p[2] > 0) & (q[2] > 0) & (u >= 0) & (u <= v.W - 1) & (w >= 0) & (w <= v.H - 1)
        px = torch.where(ok, torch.floor(u + 0.5), torch.zeros_like(u)).long()
        py = torch.where(ok, torch.floor(w + 0.5), torch.zeros_like(w)).long()
        D = v.depth.reshape(-1)[py * v.W + px]
        n_cand += ok.int()
        ok = ok & torch.isfinite(D) & (D > 0) & (p[2] <= D.double() * (1.0 + tol))
        n_pass += ok.int()
        dx, dy, dz = X0 - C[0], X1 - C[1], X2 - C[2]
        s = (dx * dx + dy * dy) / (dz * dz)
        ok = ok & torch.isfinite(s)
        k = (s.float().view(torch.int32).long() << 32) | v.id
        key = torch.minimum(key, torch.where(ok, k, torch.full_like(k, EMPTY)))
    return key, n_cand, n_pass


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--views", default="32,128")
    ap.add_argument("--size", type=int, default=2900)
    ap.add_argument("--view_size", default="2752,1856")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ortho_bench needs the GPU (no CPU timing is reported)")
    vw, vh = (int(x) for x in a.view_size.split(","))
    res = {"tool": "ortho_bench", "grid": [a.size, a.size], "unit": 0.2, "view_size": [vw, vh], "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "hbm_peak_TB_s": HBM / 1e12}
    for V in [int(x) for x in a.views.split(",")]:
        h, grid, raw = S.make_ortho_scene(a.size, a.size, 0.2, V, vw, vh, seed=V)
        views = [ortho.OrthoView(*v) for v in raw]
        cells = grid.width * grid.height
        key = ortho.select_views(h, grid, views)
        sel_ms = timed_ms(lambda: ortho.select_views(h, grid, views), a.iters)
        col_ms = timed_ms(lambda: ortho.colorize(key, h, grid, views), a.iters)
        tkey, n_cand, n_pass = torch_select(h, grid, views)
        torch.cuda.synchronize()
        t_ms = timed_ms(lambda: torch_select(h, grid, views), 1)
        cand = float(n_cand.double().mean())
        passed = float(n_pass.double().sum() / max(int(n_cand.sum()), 1))
        seen = int((key != EMPTY).sum())
        # bytes each call must move: the height and the key (read + write) once, one 4-byte depth gather per candidate
        # (a lower bound: each gather touches at least its own 4 bytes); colorize: key + height read, 4 texels per seen cell,
        # rgba + id written
        sel_bytes = cells * (4 + 8 + 8) + int(n_cand.sum()) * 4
        col_bytes = cells * (8 + 4) + seen * (4 * 4 + 4 + 4)
        res["V_%d" % V] = {
            "select_ms": round(sel_ms, 3), "colorize_ms": round(col_ms, 3),
            "candidates_per_cell": round(cand, 3), "depth_test_pass_share": round(passed, 4), "seen_cells": seen,
            "select_bytes": sel_bytes, "select_share_of_hbm": round(sel_bytes / (sel_ms * 1e-3) / HBM, 4),
            "colorize_bytes": col_bytes, "colorize_share_of_hbm": round(col_bytes / (col_ms * 1e-3) / HBM, 4),
            "torch_per_view_select_ms": round(t_ms, 3), "same_keys": bool(torch.equal(tkey, key)),
            "select_speedup_vs_torch": round(t_ms / sel_ms, 2)}
        del views, raw, h, key, tkey, n_cand, n_pass
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
