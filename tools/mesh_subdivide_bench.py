"""The mesh subdivision's kernels (csrc/mesh_subdivide.hip) at survey size: the meshes of tools/mesh_bench.py's scenes (0.5 m and
0.25 m voxels, V = 32 and V = 128 views of 2752 x 1856, about 0.2 m a pixel) subdivided against the same views.  Device-event times
(two warm-ups, mean of --iters) of every round's passes: the edge list (the adjacency and d3d_mesh_decimate_edges of the earlier
stages), measure, plan, emit; ns per (edge, view) of the measure; and a plain fp64 torch measure (advanced indexing for the depth
gathers, a view at a time) on the first --torch_edges edges of the first round, checked for equal bits.  Rows of configurations a
call does not run are kept in --out.

    python tools/mesh_subdivide_bench.py [--iters 3] [--views 32,128] [--voxels 0.5,0.25] [--max_edge 2] [--rounds 2]
        [--torch_edges 1000000] [--out profiles/mesh_subdivide_bench.json]"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_bench as MB  # noqa: E402
from deep3d_aerial_amd import mesh, subdivide  # noqa: E402


def torch_measure(vertices, edges, views, tol):
    """The comparator: subdivide.py's measure in fp64 torch, of the edges given."""
    dev = vertices.device
    X = vertices.double()
    ends = [X[edges[:, 0].long()], X[edges[:, 1].long()]]
    best = torch.zeros((edges.shape[0],), dtype=torch.float64, device=dev)
    for v in views:
        R, t, K = v.R.tolist(), v.t.tolist(), v.K.tolist()
        uv, seen = [], None
        for Q in ends:
            p = [R[r][0] * Q[:, 0] + R[r][1] * Q[:, 1] + R[r][2] * Q[:, 2] + t[r] for r in range(3)]
            g = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
            u, w = g[0] / g[2], g[1] / g[2]
            ok = (p[2] > 0) & (g[2] > 0) & (u >= 0) & (u <= v.W - 1) & (w >= 0) & (w <= v.H - 1)
            px, py = torch.floor(u + 0.5), torch.floor(w + 0.5)
            idx = torch.where(ok, py * v.W + px, torch.zeros_like(px)).long()
            D = v.depth.reshape(-1)[idx]
            ok = ok & torch.isfinite(D) & (D > 0) & (p[2] <= D.double() * (1.0 + tol))
            uv.append((u, w))
            seen = ok if seen is None else seen & ok
        du, dv = uv[0][0] - uv[1][0], uv[0][1] - uv[1][1]
        l2 = du * du + dv * dv
        best = torch.where(seen & torch.isfinite(l2) & (l2 > best), l2, best)
    return best


def timed_ms(fn, iters):
    """MB.timed_ms after one more warm-up call: a pass that allocates its outputs while the previous call's are still held
    alternates between two sets of blocks, and both are in the caching allocator only after the second call."""
    fn()
    return MB.timed_ms(fn, iters)


def run(views, voxel, iters, max_edge, rounds, torch_edges):
    grid = mesh.MeshGrid(MB.BORDER, voxel)
    v, f = mesh.depth_to_mesh(views, grid)
    tol = subdivide.DEFAULT_TOLERANCE
    row = {"views": len(views), "voxel_m": voxel, "max_edge_px": max_edge, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "rounds": []}
    out = {}
    for r in range(rounds):
        n = int(v.shape[0])
        t_edges = timed_ms(lambda: out.update(e=subdivide.edge_list(f, n)), iters)
        edges, n_edges = out["e"]
        t_measure = timed_ms(lambda: out.update(m=subdivide.measure_edges(v, edges, n_edges, views, tol)), iters)   # with the fill of the array
        measure = out["m"]
        t_plan = timed_ms(lambda: out.update(p=subdivide.plan(v, f, edges, n_edges, measure, max_edge)), iters)
        p = out["p"]
        splits, faces_out = p["totals"].cpu().tolist()
        ne = int(n_edges.item())
        rec = {"edges": ne, "seen": int((measure > 0).sum()), "longest_px": round(float(measure.max().sqrt()), 2), "split": splits,
               "faces_out": faces_out, "edge_list_ms": round(t_edges, 3), "measure_ms": round(t_measure, 3), "plan_ms": round(t_plan, 3),
               "measure_ns_per_edge_view": round(1e6 * t_measure / max(ne * len(views), 1), 4)}
        if r == 0:
            nt = min(ne, torch_edges)
            sub = edges[:nt].contiguous()
            t_torch = MB.timed_ms(lambda: out.update(t=torch_measure(v, sub, views, tol)), 1)
            rec.update(torch_edges=nt, torch_measure_ms=round(t_torch, 1), measure_ms_for_torch_edges=round(t_measure * nt / max(ne, 1), 3),
                       torch_same_bits=bool(torch.equal(out["t"].view(torch.int64), measure[:nt].view(torch.int64))))
            del sub
            out.pop("t")
        if splits:
            t_emit = timed_ms(lambda: out.update(o=subdivide.emit(v, f, n_edges, p, splits, faces_out)), iters)
            rec["emit_ms"] = round(t_emit, 3)
            v, f = out.pop("o")
        row["rounds"].append(rec)
        out.clear()
        del edges, n_edges, measure, p
        torch.cuda.empty_cache()
        if not splits:
            break
    row.update(vertices_out=int(v.shape[0]), faces_out=int(f.shape[0]))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--views", default="32,128")
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--max_edge", type=float, default=2.0, help="pixels; the scenes' voxels are 2.5 and 1.25 pixels")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--torch_edges", type=int, default=1000000, help="the torch measure runs on this many edges (the first ones)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_subdivide_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/mesh_subdivide_bench.py measures the GPU kernels: no GPU here")
    rows = []
    for nv in [int(x) for x in a.views.split(",")]:
        views = MB.make_views(nv, "cuda")
        for voxel in [float(x) for x in a.voxels.split(",")]:
            r = run(views, voxel, a.iters, a.max_edge, a.rounds, a.torch_edges)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
        del views
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "image": [MB.W, MB.H], "border": MB.BORDER, "runs": rows}
    if os.path.exists(a.out):   # rows of other configurations stay
        old = json.load(open(a.out))
        key = lambda r: (r["views"], -r["voxel_m"], r["max_edge_px"])
        done = {key(r) for r in rows}
        rows += [r for r in old.get("runs", []) if key(r) not in done]
        rows.sort(key=key)
        res = dict(old, **res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
