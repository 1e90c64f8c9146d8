"""The mesh flip (csrc/mesh_flip.hip, deep3d_aerial_amd/flip.py) on a synthetic mesh at two sizes: a --sizes N x N grid with unit
spacing, jittered by +-0.45 in x and y, z noise of sigma 0.05 and a random diagonal per cell (the mesh of tests/mesh_flip_scene.py,
larger), flipped with --max_angle 30.  Device-event times (one warm-up, median of --iters) of the passes of the first
--timed_rounds rounds: topology (adjacency + incidence + edge list), candidates, claim, apply; then the loop runs on untimed until
a round has no winner or --rounds are done.  Each pass is set against the bytes it must move, at 8 TB/s:
    candidates  40 E + 24 n + 24 m   (per edge its two ends, key and opp; once each the positions, the faces, both CSRs)
    claim       8 n + 8 E + 56 C     (the claim's fill, every key; per candidate its ends, c, d and four 8-byte atomics)
    apply       24 m + 9 E + 56 C    (the copy of the faces, every key and flag; per candidate its ends, opp and four claims)
with n vertices, m faces, E edges and C candidates.  Reported besides: candidates and winners per round, and the share of faces whose
smallest angle is below 10 and below 20 degrees before and after (tools/mesh_collapse_bench.py's sliver_share).  The comparator is
the candidates pass in plain fp64 torch on the first --torch_edges edges of the first round, checked for equal bits.  Rows of
sizes a call does not run are kept in --out.

    python tools/mesh_flip_bench.py [--iters 5] [--sizes 1024,3072] [--max_angle 30] [--rounds 64] [--timed_rounds 2]
        [--torch_edges 1000000] [--out profiles/mesh_flip_bench.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from mesh_collapse_bench import _expand, _normal, median_ms, sliver_share  # noqa: E402
from deep3d_aerial_amd import _lib, flip  # noqa: E402
from deep3d_aerial_amd._geom import ptr, stream  # noqa: E402

HASH = 2654435761
PEAK_BYTES_PER_MS = 8e9   # 8 TB/s


def grid_mesh(size, device, seed=0):
    """(vertices [size^2, 3] fp32, faces [2 (size - 1)^2, 3] int32): the jittered grid with a random diagonal per cell."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = size * size
    xy = torch.stack(torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing="xy"), -1).reshape(n, 2)
    xy = xy + (torch.rand((n, 2), generator=g, dtype=torch.float64) - 0.5) * 0.9
    z = torch.randn((n, 1), generator=g, dtype=torch.float64) * 0.05
    idx = torch.arange(n, dtype=torch.int32).reshape(size, size)
    a, b, c, d = (t.reshape(-1) for t in (idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]))
    cut = torch.rand((a.shape[0],), generator=g) < 0.5
    f0 = torch.where(cut[:, None], torch.stack([a, b, d], 1), torch.stack([a, b, c], 1))
    f1 = torch.where(cut[:, None], torch.stack([a, d, c], 1), torch.stack([b, d, c], 1))
    faces = torch.stack([f0, f1], 1).reshape(-1, 3).contiguous()
    return torch.cat([xy, z], 1).float().to(device), faces.to(device)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _d2(p, q):
    d = q - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _quality(X, i, j, k):
    """flip.py's rule 5: Q of the triangles (i, j, k), the corners taken in increasing index order."""
    idx = torch.stack([i, j, k], 1).sort(1).values
    p0, p1, p2 = X[idx[:, 0]], X[idx[:, 1]], X[idx[:, 2]]
    nrm = _normal(p0, p1, p2)
    s = (_d2(p0, p1) + _d2(p1, p2)) + _d2(p2, p0)
    return torch.where(s == 0, torch.zeros_like(s), _dot(nrm, nrm) / (s * s))


def _min(x, y):
    return torch.where(x < y, x, y)


def torch_candidates(v, f, topo, edges, max_angle):
    """The comparator: flip.py's rules 3-6 in fp64 torch for the edges given (one elementwise kernel per operation, so nothing is
    contracted): (key [E] int64, opp [E,4] int32)."""
    dev = v.device
    X, F, n = v.double(), f.long(), v.shape[0]
    offset, nbr = topo["offset"], topo["nbr"].long()
    foff, finc = topo["face_offset"].long(), topo["face_index"].long()
    E = edges.long()
    ne = E.shape[0]
    ea, eb = E[:, 0], E[:, 1]
    # (3) the pair: the faces of a's row that hold b, by the corner that follows a
    fdeg = foff[1:] - foff[:-1]
    owner, pos = _expand(foff[ea], fdeg[ea])
    fi = finc[pos]
    tri = F[fi]
    holds = (tri == eb[owner][:, None]).any(1)
    at = (tri == ea[owner][:, None]).long().argmax(1)
    nxt, prv = tri.gather(1, ((at + 1) % 3)[:, None])[:, 0], tri.gather(1, ((at + 2) % 3)[:, None])[:, 0]
    is_ab, is_ba = holds & (nxt == eb[owner]), holds & (nxt != eb[owner])
    total = lambda flag, x: torch.zeros((ne,), dtype=torch.int64, device=dev).index_add_(0, owner, torch.where(flag, x, torch.zeros_like(x)))
    one = torch.ones_like(fi)
    n_ab, n_ba = total(is_ab, one), total(is_ba, one)
    c, d, f_ab, f_ba = total(is_ab, prv), total(is_ba, nxt), total(is_ab, fi), total(is_ba, fi)   # the one value where the count is 1
    sel = ((n_ab == 1) & (n_ba == 1) & (c != d)).nonzero()[:, 0]
    a, b, c, d, f_ab, f_ba = ea[sel], eb[sel], c[sel], d[sel], f_ab[sel], f_ba[sel]
    # (4.1) the new edge by a search of the sorted (vertex, neighbour) codes, (4.2) the degrees
    deg = offset[1:] - offset[:-1]
    codes = torch.repeat_interleave(torch.arange(n, device=dev), deg) * n + nbr[:int(offset[-1])]
    query = c * n + d
    hit = torch.searchsorted(codes, query).clamp(max=max(codes.shape[0] - 1, 0))
    valid = (codes[hit] != query) & (deg[a] > 3) & (deg[b] > 3)
    # (4.3) the guard, (4.4) no face turns over, (5) the gain
    xa, xb, xc, xd = X[a], X[b], X[c], X[d]
    n1, n2 = _normal(xa, xb, xc), _normal(xb, xa, xd)
    dot = _dot(n1, n2)
    c2 = flip.cos2(max_angle)
    valid &= (dot >= 0) & (dot * dot >= c2 * (_dot(n1, n1) * _dot(n2, n2)))
    s = n1 + n2
    valid &= (_dot(_normal(xa, xd, xc), s) > 0) & (_dot(_normal(xb, xc, xd), s) > 0)
    q_old = _min(_quality(X, a, b, c), _quality(X, b, a, d))
    q_new = _min(_quality(X, a, d, c), _quality(X, b, c, d))
    valid &= q_new > q_old
    key = torch.full((ne,), -1, dtype=torch.int64, device=dev)
    opp = torch.zeros((ne, 4), dtype=torch.int32, device=dev)
    won = sel[valid]
    key[won] = (q_old[valid].float().view(torch.int32).long() << 32) | ((won * HASH) & 0xFFFFFFFF)
    opp[won] = torch.stack([c, d, f_ab, f_ba], 1)[valid].int()
    return key, opp


def pass_bytes(n, m, ne, nc):
    """The bytes each pass must move (the module docstring's table)."""
    return {"candidates": 40 * ne + 24 * n + 24 * m, "claim": 8 * n + 8 * ne + 56 * nc, "apply": 24 * m + 9 * ne + 56 * nc}


def run(size, iters, max_angle, rounds, timed_rounds, torch_edges):
    v, f = grid_mesh(size, "cuda")
    n, m = int(v.shape[0]), int(f.shape[0])
    row = {"size": size, "max_angle": max_angle, "vertices": n, "faces": m, "below_10_deg": round(sliver_share(v, f, 10.0), 4),
           "below_20_deg": round(sliver_share(v, f, 20.0), 4), "timed_rounds": []}
    per = {"edges": [], "candidates": [], "winners": []}
    out = {}
    won = True
    for r in range(min(timed_rounds, rounds)):
        t_topo = median_ms(lambda: out.update(t=flip.topology(f, n)), iters)
        topo = out["t"]
        edges, n_edges = topo["edges"], topo["n_edges"]
        csr, inc = (topo["offset"], topo["nbr"], topo["fixed"]), (topo["face_offset"], topo["face_index"])
        t_cand = median_ms(lambda: out.update(c=flip.candidates(v, f, csr, inc, edges, n_edges, max_angle)), iters)
        key, opp = out["c"]
        t_both = median_ms(lambda: out.update(w=flip.claim_apply(f, topo, key, opp)), iters)
        out_f, win, claim = out["w"]
        ne, nw = torch.cat([n_edges, topo["counts"][:1]]).cpu().tolist()
        nc = int((key >= 0).sum())
        # the claim and the apply pass one by one, through the C entry points claim_apply calls
        lib, st = _lib.load(), stream()
        emax = int(edges.shape[0])
        n_win = ctypes.c_void_p(topo["counts"].data_ptr())
        t_claim = median_ms(lambda: lib.d3d_mesh_flip_claim(n, ptr(edges), ptr(key), ptr(opp), ptr(n_edges), emax, ptr(claim), n_win, st), iters)
        t_apply = median_ms(lambda: lib.d3d_mesh_flip_apply(ptr(f), m, ptr(edges), ptr(key), ptr(opp), ptr(n_edges), emax, ptr(claim), ptr(out_f),
                                                            ptr(win), n_win, st), iters)
        nbytes = pass_bytes(n, m, ne, nc)
        rec = {"edges": ne, "candidates": nc, "winners": nw, "topology_ms": round(t_topo, 3), "candidates_ms": round(t_cand, 3),
               "claim_ms": round(t_claim, 3), "apply_ms": round(t_apply, 3), "claim_apply_with_allocations_ms": round(t_both, 3),
               "round_ms": round(t_topo + t_cand + t_both, 3), "bytes": nbytes,
               "candidates_x_bytes_at_8TBs": round(t_cand * PEAK_BYTES_PER_MS / nbytes["candidates"], 2),
               "claim_x_bytes_at_8TBs": round(t_claim * PEAK_BYTES_PER_MS / nbytes["claim"], 2),
               "apply_x_bytes_at_8TBs": round(t_apply * PEAK_BYTES_PER_MS / nbytes["apply"], 2)}
        if r == 0:
            nt = min(ne, torch_edges)
            sub = edges[:nt].contiguous()
            t_torch = median_ms(lambda: out.update(x=torch_candidates(v, f, topo, sub, max_angle)), 1)
            tk, to = out.pop("x")
            rec.update(torch_edges=nt, torch_candidates_ms=round(t_torch, 1), candidates_ms_for_torch_edges=round(t_cand * nt / max(ne, 1), 3),
                       torch_same_bits=bool(torch.equal(tk, key[:nt]) and torch.equal(to, opp[:nt])))
            del sub, tk, to
        for name, x in (("edges", ne), ("candidates", nc), ("winners", nw)):
            per[name].append(x)
        row["timed_rounds"].append(rec)
        won = nw > 0
        if won:
            f = out_f.clone()
        out.clear()
        del topo, edges, n_edges, csr, inc, key, opp, out_f, win, claim
        torch.cuda.empty_cache()
        if not won:
            break
    left = rounds - len(per["winners"])
    hit = won and left == 0
    if won and left > 0:
        info = {}
        v, f = flip.flip_edges(v, f, max_angle, rounds=left, info=info)
        for name in per:
            per[name] += info[name]
        hit = info["hit_max_rounds"]
    row.update(per, rounds=len(per["winners"]), hit_max_rounds=hit, flips=sum(per["winners"]),
               below_10_deg_out=round(sliver_share(v, f, 10.0), 4), below_20_deg_out=round(sliver_share(v, f, 20.0), 4))
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", default="1024,3072", help="the grids' side lengths in vertices")
    ap.add_argument("--max_angle", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=flip.MAX_ROUNDS, help="the cap on the rounds run until no winner")
    ap.add_argument("--timed_rounds", type=int, default=2, help="the first rounds, whose passes are timed one by one")
    ap.add_argument("--torch_edges", type=int, default=1000000, help="the torch candidates run on this many edges (the first ones)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_flip_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/mesh_flip_bench.py measures the GPU kernels: no GPU here")
    rows = []
    for size in [int(x) for x in a.sizes.split(",")]:
        r = run(size, a.iters, a.max_angle, a.rounds, a.timed_rounds, a.torch_edges)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "runs": rows}
    if os.path.exists(a.out):   # rows of other sizes stay
        old = json.load(open(a.out))
        key = lambda r: (r["size"], r["max_angle"])
        done = {key(r) for r in rows}
        rows += [r for r in old.get("runs", []) if key(r) not in done]
        rows.sort(key=key)
        res = dict(old, **res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
