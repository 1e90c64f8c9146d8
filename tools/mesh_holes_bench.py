"""The hole-closing kernels (csrc/mesh_holes.hip) at survey size: the 600 x 600 m scene of tools/mesh_bench.py (ground and 120
box buildings, 32 views of 2752 x 1856) meshed at 0.5 m voxels.  Every view sees almost the whole scene, so a dropped pixel
leaves no hole in the mesh; the dropouts here are discs on the ground plane (radius 0.4 - 4 m) inside which every view loses its
depth, as an occluder or a low-confidence region would have it, plus the 2 % of single pixels of tools/mesh_clean_bench.py.
Device-event times (median of 5 after a warm-up) of the passes: the vertex -> face incidence, boundary, loops (hooking + pointer
jumping, the host reading one flag per round), plan (the walks and the two scans; its read of the totals included), emit, the
whole close_holes, and the full clean of the same mesh (removal, one smoothing iteration) without and with the step; the loops,
the holes closed and the rounds.  Prints one JSON line (and writes --out).

    python tools/mesh_holes_bench.py [--voxel 0.5] [--views 32] [--discs 1500] [--max_edges 30] [--out profiles/mesh_holes_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mesh_bench as MB  # noqa: E402
import mesh_clean_bench as CB  # noqa: E402
from deep3d_aerial_amd import mesh  # noqa: E402

CELL = 0.25   # the dropout mask's cell, in metres


def dropout_mask(n_discs, dev, seed=11):
    """[rows, cols] bool over the scene's x, y extent at CELL: inside a disc."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = MB.BORDER[:4]
    cols, rows = int((x1 - x0) / CELL), int((y1 - y0) / CELL)
    mask = torch.zeros((rows, cols), dtype=torch.bool, device=dev)
    ys, xs = torch.meshgrid(torch.arange(rows, device=dev), torch.arange(cols, device=dev), indexing="ij")
    for _ in range(n_discs):
        cx, cy, r = rng.uniform(x0 + 5, x1 - 5), rng.uniform(y0 + 5, y1 - 5), rng.uniform(0.4, 4.0)
        i0, i1 = max(int((cy - r - y0) / CELL), 0), min(int((cy + r - y0) / CELL) + 2, rows)
        j0, j1 = max(int((cx - r - x0) / CELL), 0), min(int((cx + r - x0) / CELL) + 2, cols)
        yy = y0 + (ys[i0:i1, j0:j1].double() + 0.5) * CELL
        xx = x0 + (xs[i0:i1, j0:j1].double() + 0.5) * CELL
        mask[i0:i1, j0:j1] |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    return mask


def drop(view, mask):
    """Zeroes the depth of every pixel whose surface point lies over a masked cell."""
    dev = view.depth.device
    H, W = view.H, view.W
    K = torch.tensor(view.K, dtype=torch.float64, device=dev)
    R, t = torch.tensor(view.R, dtype=torch.float64, device=dev), torch.tensor(view.t, dtype=torch.float64, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.linalg.inv(K) @ torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64, device=dev)])
    X = (R.T @ (dc * view.depth.reshape(1, -1).double() - t[:, None])).T     # the camera z of the ray is 1: the parameter is the depth
    x0, _, y0, _ = MB.BORDER[:4]
    j = ((X[:, 0] - x0) / CELL).floor().long()
    i = ((X[:, 1] - y0) / CELL).floor().long()
    ok = (i >= 0) & (i < mask.shape[0]) & (j >= 0) & (j < mask.shape[1]) & (view.depth.reshape(-1) > 0)
    hit = torch.zeros(H * W, dtype=torch.bool, device=dev)
    hit[ok] = mask[i[ok], j[ok]]
    view.depth[hit.reshape(H, W)] = 0.0


def run(voxel, views, max_edges):
    V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(MB.BORDER, voxel))
    n, m = int(V.shape[0]), int(F.shape[0])
    info = {}
    V2, F2 = mesh.close_holes(V, F, max_edges, info=info)
    inc = mesh.face_incidence(F, n)
    b = mesh._boundary(F, n, inc)
    d = mesh._loops(F, n, dict(b))
    p = mesh._plan_holes(V, F, n, m, max_edges, loops=d)
    V3, F3 = mesh.close_holes(V, F, max_edges)
    again = {}
    mesh.close_holes(V2, F2, max_edges, info=again)
    cinfo = {}
    Vc, Fc = mesh.clean(V, F, CB.MIN_FACES, CB.SPURIOUS, 1, close_holes=max_edges, info=cinfo)
    fixed = lambda f_, n_: int(mesh.adjacency(f_, n_)[2].sum())

    def emit():
        out_v = torch.empty((n + p["holes"], 3), dtype=torch.float32, device=V.device)
        out_f = torch.empty((m + p["faces_added"], 3), dtype=torch.int32, device=V.device)
        g = mesh._ptr
        mesh._lib.check(mesh._lib.load().d3d_mesh_holes_emit(g(V), n, g(F), m, g(p["successor"]), g(p["label"]), g(p["qualify"]), g(p["position"]),
                                                             g(p["vertex_offset"]), g(p["face_offset"]), g(p["centroid"]), p["holes"],
                                                             p["faces_added"], g(out_v), g(out_f), mesh._stream()), "d3d_mesh_holes_emit")

    count = d["count"][:n]
    res = {
        "voxel": voxel, "max_edges": max_edges, "vertices": n, "triangles": m, "boundary_half_edges": int(b["boundary"].sum()),
        "loops": info["loops"], "holes_closed": info["holes_closed"], "faces_added": info["faces_added"],
        "skipped_outer": info["skipped_outer"], "skipped_large": info["skipped_large"], "skipped_not_simple": info["skipped_not_simple"],
        "rounds": info["rounds"], "longest_loop": int(count.max()) if n else 0, "second_call_closes": again["holes_closed"],
        "same_bits_run_to_run": bool(torch.equal(V2.view(torch.int32), V3.view(torch.int32)) and torch.equal(F2, F3)),
        "fixed_vertices_before": fixed(F, n), "fixed_vertices_after": fixed(F2, int(V2.shape[0])),
        "clean_with_step_holes_closed": cinfo["close_holes"]["holes_closed"],
        "incidence_ms": CB.median_ms(lambda: mesh.face_incidence(F, n)),
        "boundary_ms": CB.median_ms(lambda: mesh._boundary(F, n, inc)),
        "loops_ms": CB.median_ms(lambda: mesh._loops(F, n, dict(b))),
        "plan_ms": CB.median_ms(lambda: mesh._plan_holes(V, F, n, m, max_edges, loops=d)),
        "emit_ms": CB.median_ms(emit) if p["holes"] else 0.0,
        "close_holes_ms": CB.median_ms(lambda: mesh.close_holes(V, F, max_edges)),
        "full_clean_ms": CB.median_ms(lambda: mesh.clean(V, F, CB.MIN_FACES, CB.SPURIOUS, 1)),
        "full_clean_with_close_holes_ms": CB.median_ms(lambda: mesh.clean(V, F, CB.MIN_FACES, CB.SPURIOUS, 1, close_holes=max_edges)),
    }
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--voxel", type=float, default=0.5)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--discs", type=int, default=1500)
    ap.add_argument("--max_edges", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.cuda.set_device(0)
    views = CB.make_views(a.views, 0, "cuda")
    mask = dropout_mask(a.discs, "cuda")
    for v in views:
        drop(v, mask)
    out = {"tool": "mesh_holes_bench", "views": a.views, "discs": a.discs, "min_faces": CB.MIN_FACES, "spurious": CB.SPURIOUS,
           "device": torch.cuda.get_device_name(0), "runs": [run(a.voxel, views, a.max_edges)]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
