"""The mesh refinement's kernels (csrc/mesh_refine.hip) at survey size: the meshes of tools/mesh_bench.py's scenes (0.5 m and 0.25 m
voxels, V = 32 and V = 128 views of 2752 x 1856) refined against the same views with tools/texture_bench.py's synthetic images,
step = spacing = half the voxel, every other setting at its default.  Device-event times (one warm-up, mean of --iters) of one
scale's passes: topology (the two CSRs of the earlier stages), frames, view lists, match, relax, apply; the counters; and a plain
fp64 torch match (advanced indexing for the gathers, a view at a time) on the first --torch_vertices vertices, checked for the same
pick.  With --variant_library SO (a `make REFINE=per_hypothesis` build) the entry also holds `mappings`: the match of both builds on the
same tensors, taking turns.  --min_contrast 0.01 lets nearly every vertex sweep every hypothesis in all its views; at the
stage's default of 2 grey levels the bench's smooth ramps stop most vertices after one patch.  The images here are a function of the pixel and differ from view to view, so few vertices find a
correlation above min_score: the counts say what the kernels did, not what the rule is worth (tests/test_mesh_refine.py measures
that).  Rows of configurations a call does not run are kept in --out.

    python tools/mesh_refine_bench.py [--iters 3] [--views 32,128] [--voxels 0.5,0.25] [--torch_vertices 200000]
        [--min_contrast C] [--variant_library SO] [--out profiles/mesh_refine_bench.json]"""
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

import mesh_bench as MB  # noqa: E402
import texture_bench as TB  # noqa: E402
from deep3d_aerial_amd import mesh, refine  # noqa: E402


def torch_match(vertices, frame, active, lists, views, reach, step, spacing, min_score, min_contrast, chunk=32768):
    """The comparator: refine.py's sweep and pick in fp64 torch.  (kstar, weight, d0) of the vertices given."""
    dev = vertices.device
    n, nk = int(vertices.shape[0]), 2 * reach + 1
    Tv = refine.min_variance(min_contrast)
    kstar = torch.full((n,), -1, dtype=torch.int32, device=dev)
    weight, d0 = torch.zeros((n,), device=dev), torch.zeros((n,), device=dev)
    h = (torch.arange(nk, device=dev) - reach).double() * step
    pa = ((torch.arange(25, device=dev) % 5) - 2).double() * spacing
    pb = ((torch.arange(25, device=dev) // 5) - 2).double() * spacing
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(c0 + chunk, n))
        X, fr, keys = vertices[sl].double(), frame[sl], lists[sl]
        two = active[sl].bool() & (keys[:, 1] != refine.EMPTY_KEY)
        Xk = X[:, None, :] + h[None, :, None] * fr[:, None, 0:3]
        P = (Xk[:, :, None, :] + pa[None, None, :, None] * fr[:, None, None, 3:6]) + pb[None, None, :, None] * fr[:, None, None, 6:9]
        c = P.shape[0]
        q = torch.zeros((refine.VIEWS, c, nk, 25), dtype=torch.int64, device=dev)
        ok = torch.zeros((refine.VIEWS, c, nk), dtype=torch.bool, device=dev)
        ids = keys & 0xffffffff
        for v in views:
            R, t, K = v.R.tolist(), v.t.tolist(), v.K.tolist()
            img = v.rgba.reshape(-1, 4)
            for s in range(refine.VIEWS):
                sel = torch.nonzero(two & (keys[:, s] != refine.EMPTY_KEY) & (ids[:, s] == v.id))[:, 0]
                if not sel.numel():
                    continue
                Q = P[sel]
                p = [R[r][0] * Q[..., 0] + R[r][1] * Q[..., 1] + R[r][2] * Q[..., 2] + t[r] for r in range(3)]
                g = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
                u, w = g[0] / g[2], g[1] / g[2]
                good = (p[2] > 0) & (g[2] > 0) & (u >= 0) & (u <= v.W - 1) & (w >= 0) & (w <= v.H - 1)
                u, w = torch.where(good, u, torch.zeros_like(u)), torch.where(good, w, torch.zeros_like(w))
                fu, fw = torch.floor(u), torch.floor(w)
                fx, fy = (u - fu)[..., None], (w - fw)[..., None]
                x0, y0 = fu.clamp(0, v.W - 1).long(), fw.clamp(0, v.H - 1).long()
                x1, y1 = (x0 + 1).clamp(max=v.W - 1), (y0 + 1).clamp(max=v.H - 1)
                tex = lambda y, x: img[y * v.W + x, :3].double()
                tap = (((1.0 - fx) * (1.0 - fy) * tex(y0, x0) + fx * (1.0 - fy) * tex(y0, x1)) + (1.0 - fx) * fy * tex(y1, x0)) + \
                    fx * fy * tex(y1, x1)
                grey = torch.floor(4.0 * ((tap[..., 0] + tap[..., 1]) + tap[..., 2]) + 0.5).clamp(0, 3060).long()
                q[s, sel] = torch.where(good, grey, torch.zeros_like(grey))
                ok[s, sel] = good.all(-1)
        S, SS = q.sum(-1), (q * q).sum(-1)
        var = 25 * SS - S * S
        z = torch.zeros((c, nk, 3), dtype=torch.float64, device=dev)
        pair = torch.zeros((c, nk, 3), dtype=torch.bool, device=dev)
        for j in range(1, refine.VIEWS):
            num = 25 * (q[0] * q[j]).sum(-1) - S[0] * S[j]
            good = ok[0] & ok[j] & (var[0] >= Tv) & (var[j] >= Tv)
            zj = num.double() / torch.sqrt(var[0].double() * var[j].double())
            z[:, :, j - 1], pair[:, :, j - 1] = torch.where(good, zj, torch.zeros_like(zj)), good
        used = pair.all(1) & two[:, None]
        score = torch.zeros((c, nk), dtype=torch.float64, device=dev)
        for j in range(3):
            score = score + torch.where(used[:, None, j], z[:, :, j], torch.zeros_like(score))
        cnt = used.sum(1)
        has = cnt > 0
        score = score / cnt.clamp(min=1)[:, None].double()
        # the pick: largest score, then smaller |k - reach|, then smaller k
        best = score.max(1).values
        kk = torch.arange(nk, device=dev)
        rank = torch.where(score == best[:, None], (kk - reach).abs() * 2 * nk + kk, torch.full_like(kk, 1 << 30))
        k = rank.argmin(1)
        idx = torch.arange(c, device=dev)
        sm, sp = score[idx, (k - 1).clamp(min=0)], score[idx, (k + 1).clamp(max=nk - 1)]
        den = (sm - 2.0 * best) + sp
        inner = (k > 0) & (k < nk - 1) & (den < 0)
        delta = torch.where(inner, (0.5 * (sm - sp) / torch.where(inner, den, torch.ones_like(den))).clamp(-0.5, 0.5), torch.zeros_like(den))
        kstar[sl] = torch.where(has, k, torch.full_like(k, -1)).int()
        weight[sl] = torch.where(has & ~(best < min_score), 1.0, 0.0).float()
        d0[sl] = torch.where(has, (((k - reach).double() + delta) * step), torch.zeros_like(delta)).float()
    return kstar, weight, d0


def run(views, voxel, iters, torch_vertices, variant=None, min_contrast=None):
    grid = mesh.MeshGrid(MB.BORDER, voxel)
    vertices, faces = mesh.depth_to_mesh(views, grid)
    ov = TB.ortho_views(views)
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    s = refine.check_refine_settings({"step": voxel / 2, "min_contrast": min_contrast})
    step, spacing, reach = s["step"], s["spacing"], s["reach"]
    out = {}
    t_topo = MB.timed_ms(lambda: out.update(t=refine.Topology(faces, n)), iters)
    topo = out["t"]
    t_frames = MB.timed_ms(lambda: out.update(f=refine.vertex_frames(vertices, faces, topo)), iters)
    frame, active = out["f"]
    t_views = MB.timed_ms(lambda: out.update(l=refine.vertex_views(vertices, frame, active, ov, step, reach)), iters)   # with the fill of the list
    lists = out["l"]
    t_match = MB.timed_ms(lambda: out.update(m=refine.match(vertices, frame, active, lists, ov, step, spacing, reach, s["min_score"],
                                                            s["min_contrast"])), iters)
    kstar, weight, d0, counts = out["m"]
    t_relax = MB.timed_ms(lambda: out.update(d=refine.relax(weight, d0, active, topo, s["smooth"], s["smooth_iterations"])), iters)
    t_apply = MB.timed_ms(lambda: refine.apply(vertices, frame, active, out["d"]), iters)
    c = counts.cpu().tolist()
    nt = min(n, torch_vertices)
    sub = lambda x: x[:nt].contiguous()
    t_torch = MB.timed_ms(lambda: out.update(tm=torch_match(sub(vertices), sub(frame), sub(active), sub(lists), ov, reach, step, spacing,
                                                            s["min_score"], s["min_contrast"])), 1)
    tk, tw, td = out["tm"]
    row = {"views": len(ov), "voxel_m": voxel, "min_contrast": s["min_contrast"], "match_ms_mapping": "per_vertex", "vertices": n, "faces": m, "step": step, "spacing": spacing, "reach": reach,
           "active": c[0], "two_views": c[1], "matched": c[2], "moved": c[3], "topology_ms": round(t_topo, 3), "frames_ms": round(t_frames, 3),
           "views_ms": round(t_views, 3), "match_ms": round(t_match, 3), "relax_ms": round(t_relax, 3), "relax_iterations": s["smooth_iterations"],
           "apply_ms": round(t_apply, 3), "match_ns_per_swept_vertex": round(1e6 * t_match / max(c[1], 1), 2),
           "gathers": c[1] * (2 * reach + 1) * 25 * 4 * 4, "torch_vertices": nt, "torch_match_ms": round(t_torch, 1),
           "match_ms_for_torch_vertices": round(t_match * nt / n, 3),
           "torch_same_pick": bool(torch.equal(tk, kstar[:nt]) and torch.equal(tw, weight[:nt]) and torch.equal(td, d0[:nt]))}
    if variant is not None:
        other = ctypes.CDLL(variant)
        other.d3d_mesh_refine_match.argtypes = refine._lib.SIGNATURES["d3d_mesh_refine_match"]
        other.d3d_mesh_refine_match.restype = ctypes.c_int
        libs = {"per_vertex": refine._lib.load(), "per_hypothesis": other}
        P = refine._ptr
        recs, nr = refine._table(ov, vertices.device)
        res = {k: (torch.empty_like(kstar), torch.empty_like(weight), torch.empty_like(d0), torch.zeros_like(counts)) for k in libs}

        def call(k):
            ks, w, d, cn = res[k]
            rc = libs[k].d3d_mesh_refine_match(P(vertices), n, P(frame), P(active), P(lists), P(recs), nr, reach, step, spacing,
                                               refine.min_variance(s["min_contrast"]), s["min_score"], P(ks), P(w), P(d), P(cn), refine._stream())
            if rc != 0:
                raise RuntimeError("d3d_mesh_refine_match of the %s build: %d" % (k, rc))

        times = {k: [] for k in libs}
        for _ in range(3):
            for k in libs:
                times[k].append(round(MB.timed_ms(lambda: call(k), iters), 3))
        same = all(torch.equal(a, b) and torch.equal(a, want) for a, b, want in zip(res["per_hypothesis"], res["per_vertex"],
                                                                                   (kstar, weight, d0, counts)))
        row["mappings"] = {"per_hypothesis_ms": times["per_hypothesis"], "per_vertex_ms": times["per_vertex"], "same_bits": bool(same)}
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--views", default="32,128")
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--torch_vertices", type=int, default=200000, help="the torch match runs on this many vertices (the first ones)")
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="a REFINE=per_hypothesis build of the library whose match is timed beside this one")
    ap.add_argument("--min_contrast", type=float, default=None,
                    help="the contrast floor (default: the stage's 2 grey levels, which the bench's smooth ramps mostly miss, so most vertices "
                         "stop after one patch; 0.01 lets nearly every vertex sweep every hypothesis in all its views)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_refine_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/mesh_refine_bench.py measures the GPU kernels: no GPU here")
    rows = []
    for nv in [int(x) for x in a.views.split(",")]:
        views = MB.make_views(nv, "cuda")
        for voxel in [float(x) for x in a.voxels.split(",")]:
            r = run(views, voxel, a.iters, a.torch_vertices, a.variant_library, a.min_contrast)
            print(json.dumps(r), flush=True)
            rows.append(r)
            torch.cuda.empty_cache()
        del views
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "image": [MB.W, MB.H], "border": MB.BORDER, "runs": rows}
    if os.path.exists(a.out):   # rows of other configurations stay
        old = json.load(open(a.out))
        key = lambda r: (r["views"], -r["voxel_m"], -r.get("min_contrast", refine.DEFAULT_MIN_CONTRAST))
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
