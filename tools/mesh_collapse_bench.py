"""The mesh collapse (csrc/mesh_collapse.hip, deep3d_aerial_amd/collapse.py) at survey size: the meshes of tools/mesh_bench.py's
scene (0.5 m and 0.25 m voxels, views of 2752 x 1856, about 0.2 m a pixel) collapsed against the same views, min_edge 1 pixel.
Device-event times (one warm-up, median of --iters) of the passes of the first --timed_rounds rounds: adjacency + incidence + edge
list, measure, candidates, claim + apply, faces + compact; then the loop runs on untimed until a round has no winner or --rounds
are done.  Reported besides: edges, short edges, valid candidates and winners per round, faces and vertices before and after, and
the share of faces whose smallest angle is below 10 degrees before and after, the stage's visible benefit.  The comparator is the
candidates pass in plain fp64 torch on the first --torch_edges edges of the first round, checked for equal bits.  Rows of
configurations a call does not run are kept in --out.

    python tools/mesh_collapse_bench.py [--iters 5] [--views 32] [--voxels 0.5,0.25] [--min_edge 1] [--max_edge 4] [--rounds 64]
        [--timed_rounds 2] [--torch_edges 1000000] [--out profiles/mesh_collapse_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_bench as MB  # noqa: E402
from deep3d_aerial_amd import collapse, mesh, subdivide  # noqa: E402

HASH = 2654435761


def median_ms(fn, iters):
    """Device-event milliseconds of fn: one warm-up call, then the median of `iters` calls timed one by one."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def sliver_share(v, f, degrees=10.0):
    """The share of faces whose smallest angle is below `degrees` (a face of no area counts), in fp64 torch."""
    if f.shape[0] == 0:
        return 0.0
    p = v.double()[f.long()]
    smallest = None
    for i in range(3):
        a, b = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        c = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))
        ang = torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)))
        ang = torch.where(torch.isfinite(ang), ang, torch.zeros_like(ang))
        smallest = ang if smallest is None else torch.minimum(smallest, ang)
    return float((smallest < degrees).double().mean())


def _expand(start, length):
    """owner and position of every entry of the rows (start, length)."""
    owner = torch.repeat_interleave(torch.arange(start.shape[0], device=start.device), length)
    first = torch.cumsum(length, 0) - length
    pos = torch.arange(owner.shape[0], device=start.device) - first[owner] + start[owner]
    return owner, pos


def _normal(p0, p1, p2):
    u, w = p1 - p0, p2 - p0
    return torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def _d2(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def torch_candidates(v, f, topo, edges, measure, min_edge, max_edge):
    """The comparator: collapse.py's rule 4 in fp64 torch for the edges given (one elementwise kernel per operation, so nothing is
    contracted): (target [E,3] fp32, key [E] int64)."""
    dev = v.device
    X, F, n = v.double(), f.long(), v.shape[0]
    offset, nbr, fixed = topo["offset"], topo["nbr"].long(), topo["fixed"]
    foff, finc = topo["face_offset"].long(), topo["face_index"].long()
    E = edges.long()
    min2, max2 = min_edge * min_edge, max_edge * max_edge
    cand = (measure > 0) & (measure < min2) & ~((fixed[E[:, 0]] != 0) & (fixed[E[:, 1]] != 0))
    sel = cand.nonzero()[:, 0]
    ea, eb, m = E[sel, 0], E[sel, 1], measure[sel]
    fa, fb = fixed[ea] != 0, fixed[eb] != 0
    k = sel.shape[0]
    count = lambda owner, flag: torch.zeros((k,), dtype=torch.int64, device=dev).index_add_(0, owner, flag.long())
    deg = offset[1:] - offset[:-1]
    # (1) the link condition by a search of the sorted (vertex, neighbour) codes, (2) the degree
    codes = torch.repeat_interleave(torch.arange(n, device=dev), deg) * n + nbr[:int(offset[-1])]
    owner, pos = _expand(offset[ea], deg[ea])
    query = eb[owner] * n + nbr[pos]
    at = torch.searchsorted(codes, query).clamp(max=max(codes.shape[0] - 1, 0))
    valid = (count(owner, codes[at] == query) == 2) & (deg[ea] + deg[eb] - 4 >= 3)
    xa, xb = X[ea], X[eb]
    t32 = torch.where(fa[:, None], v[ea], torch.where(fb[:, None], v[eb], ((xa + xb) * 0.5).float()))
    t = t32.double()
    s = m / _d2(xb, xa)
    fdeg = foff[1:] - foff[:-1]
    for row, other in ((ea, eb), (eb, ea)):
        # (4) the guard over the row's neighbours
        owner, pos = _expand(offset[row], deg[row])
        w = nbr[pos]
        bad = (w != other[owner]) & ~(_d2(t[owner], X[w]) * s[owner] <= max2)
        valid &= count(owner, bad) == 0
        # (3) the flips over the row's faces
        owner, pos = _expand(foff[row], fdeg[row])
        tri = F[finc[pos]]
        p = X[tri]
        n0 = _normal(p[:, 0], p[:, 1], p[:, 2])
        p = torch.where((tri == row[owner][:, None])[:, :, None], t[owner][:, None, :], p)
        n1 = _normal(p[:, 0], p[:, 1], p[:, 2])
        dot = (n0[:, 0] * n1[:, 0] + n0[:, 1] * n1[:, 1]) + n0[:, 2] * n1[:, 2]
        bad = ~(tri == other[owner][:, None]).any(1) & ~(dot > 0)
        valid &= count(owner, bad) == 0
    target = torch.zeros((E.shape[0], 3), dtype=torch.float32, device=dev)
    key = torch.full((E.shape[0],), -1, dtype=torch.int64, device=dev)
    won = sel[valid]
    target[won] = t32[valid]
    key[won] = (m[valid].float().view(torch.int32).long() << 32) | ((won * HASH) & 0xFFFFFFFF)
    return target, key


def run(views, voxel, iters, min_edge, max_edge, rounds, timed_rounds, torch_edges):
    grid = mesh.MeshGrid(MB.BORDER, voxel)
    v, f = mesh.depth_to_mesh(views, grid)
    tol = collapse.DEFAULT_TOLERANCE
    row = {"views": len(views), "voxel_m": voxel, "min_edge_px": min_edge, "max_edge_px": max_edge, "vertices": int(v.shape[0]),
           "faces": int(f.shape[0]), "sliver_share": round(sliver_share(v, f), 4), "timed_rounds": []}
    per = {"edges": [], "short": [], "valid": [], "winners": []}
    out = {}
    won = True
    for r in range(min(timed_rounds, rounds)):
        n = int(v.shape[0])
        t_topo = median_ms(lambda: out.update(t=collapse.topology(f, n)), iters)
        topo = out["t"]
        edges, n_edges = topo["edges"], topo["n_edges"]
        csr, inc = (topo["offset"], topo["nbr"], topo["fixed"]), (topo["face_offset"], topo["face_index"])
        t_measure = median_ms(lambda: out.update(m=subdivide.measure_edges(v, edges, n_edges, views, tol)), iters)   # with the fill of the array
        measure = out["m"]
        t_cand = median_ms(lambda: out.update(c=collapse.candidates(v, f, csr, inc, edges, n_edges, measure, min_edge, max_edge)), iters)
        target, key = out["c"]
        t_claim = median_ms(lambda: out.update(w=collapse.claim_apply(v, topo, target, key)), iters)
        moved, remap, win, _ = out["w"]
        t_faces = median_ms(lambda: out.update(o=collapse.faces_compact(moved, f, remap, topo["counts"])), iters)
        ne, nw, mk, nk = torch.cat([n_edges, topo["counts"]]).cpu().tolist()
        n_short, n_valid = int(((measure > 0) & (measure < min_edge * min_edge)).sum()), int((key >= 0).sum())
        rec = {"edges": ne, "short": n_short, "valid": n_valid, "winners": nw, "topology_ms": round(t_topo, 3), "measure_ms": round(t_measure, 3),
               "candidates_ms": round(t_cand, 3), "claim_apply_ms": round(t_claim, 3), "faces_compact_ms": round(t_faces, 3),
               "candidates_ns_per_edge": round(1e6 * t_cand / max(ne, 1), 4),
               "candidates_ns_per_short_edge": round(1e6 * t_cand / max(n_short, 1), 4)}
        if r == 0:
            nt = min(ne, torch_edges)
            sub, msub = edges[:nt].contiguous(), measure[:nt].contiguous()
            t_torch = median_ms(lambda: out.update(x=torch_candidates(v, f, topo, sub, msub, min_edge, max_edge)), 1)
            tt, tk = out.pop("x")
            rec.update(torch_edges=nt, torch_candidates_ms=round(t_torch, 1), candidates_ms_for_torch_edges=round(t_cand * nt / max(ne, 1), 3),
                       torch_same_bits=bool(torch.equal(tk, key[:nt]) and torch.equal(tt.view(torch.int32), target[:nt].view(torch.int32))))
            del sub, msub, tt, tk
        for name, x in (("edges", ne), ("short", n_short), ("valid", n_valid), ("winners", nw)):
            per[name].append(x)
        row["timed_rounds"].append(rec)
        out_v, out_f = out.pop("o")
        won = nw > 0
        if won:
            v, f = out_v[:nk].clone(), out_f[:mk].clone()
        out.clear()
        del topo, edges, n_edges, csr, inc, measure, target, key, moved, remap, win, out_v, out_f
        torch.cuda.empty_cache()
        if not won:
            break
    left = rounds - len(per["winners"])
    hit = won and left == 0
    if won and left > 0:
        info = {}
        v, f = collapse.collapse(v, f, views, min_edge, max_edge, rounds=left, info=info)
        for name in per:
            per[name] += info[name]
        hit = info["hit_max_rounds"]
    row.update(per, rounds=len(per["winners"]), hit_max_rounds=hit, vertices_out=int(v.shape[0]), faces_out=int(f.shape[0]),
               sliver_share_out=round(sliver_share(v, f), 4))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--views", default="32")
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--min_edge", type=float, default=1.0, help="pixels; the scenes' voxels are 2.5 and 1.25 pixels")
    ap.add_argument("--max_edge", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=collapse.MAX_ROUNDS, help="the cap on the rounds run until no winner")
    ap.add_argument("--timed_rounds", type=int, default=2, help="the first rounds, whose passes are timed one by one")
    ap.add_argument("--torch_edges", type=int, default=1000000, help="the torch candidates run on this many edges (the first ones)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_collapse_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/mesh_collapse_bench.py measures the GPU kernels: no GPU here")
    rows = []
    for nv in [int(x) for x in a.views.split(",")]:
        views = MB.make_views(nv, "cuda")
        for voxel in [float(x) for x in a.voxels.split(",")]:
            r = run(views, voxel, a.iters, a.min_edge, a.max_edge, a.rounds, a.timed_rounds, a.torch_edges)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
        del views
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "image": [MB.W, MB.H], "border": MB.BORDER, "runs": rows}
    if os.path.exists(a.out):   # rows of other configurations stay
        old = json.load(open(a.out))
        key = lambda r: (r["views"], -r["voxel_m"], r["min_edge_px"])
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
