"""The mesh kernels (csrc/mesh.hip) at survey size: a 600 x 600 x 150 m grid of synthetic ground plus box buildings at 0.5 m and
0.25 m voxels, V = 32 and V = 128 views of 2752 x 1856 from 400-600 m up (half nadir, half oblique), depth maps ray-cast on the
GPU (torch, this tool only) with 2 % holes and a confidence of 0.9.  Device-event time of the allocation (mark + bricks), the
integration and the extraction (count + emit + compact); the allocated bricks, the vertex and triangle counts, and the mean
number of views that observe an observed voxel.  The comparator is the same integration written in fp64 torch over the
allocated voxels, one view at a time; both must give the same sums and counts.  Prints one JSON line (and writes --out).

    python tools/mesh_bench.py [--iters 3] [--views 32,128] [--voxels 0.5,0.25] [--out profiles/mesh_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep3d_aerial_amd import mesh  # noqa: E402

W, H = 2752, 1856
BORDER = [-300.0, 300.0, -300.0, 300.0, -20.0, 130.0]


def boxes(seed=0, n=120):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(-280, 280, 2)
        sx, sy = rng.uniform(8, 40, 2)
        out.append((cx - sx / 2, cx + sx / 2, cy - sy / 2, cy + sy / 2, rng.uniform(5, 90)))
    return out


def look_at(C, T):
    f = np.asarray(T, np.float64) - C
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r = r / np.linalg.norm(r) if np.linalg.norm(r) > 1e-9 else np.array([1.0, 0.0, 0.0])
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ C
    return E.astype(np.float32)


def render(K, E, bx, dev, rng):
    """Depth [H,W] fp32 of ground z = 0 plus boxes, ray-cast in fp64 torch; 2 % holes."""
    K64, E64 = torch.tensor(K, dtype=torch.float64, device=dev), torch.tensor(E, dtype=torch.float64, device=dev)
    R, t = E64[:3, :3], E64[:3, 3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.linalg.inv(K64) @ torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64, device=dev)])
    d = (R.T @ dc).T
    C = -R.T @ t
    lam = torch.where(d[:, 2] < 0, -C[2] / d[:, 2], torch.full_like(d[:, 2], math.inf))
    for x0, x1, y0, y1, z1 in bx:
        lo = torch.tensor([x0, y0, 0.0], dtype=torch.float64, device=dev)
        hi = torch.tensor([x1, y1, z1], dtype=torch.float64, device=dev)
        t0, t1 = (lo - C) / d, (hi - C) / d
        tn = torch.minimum(t0, t1).nan_to_num(-math.inf).amax(1)
        tf = torch.maximum(t0, t1).nan_to_num(math.inf).amin(1)
        lam = torch.where((tn <= tf) & (tn > 0), torch.minimum(lam, tn), lam)
    lam = torch.where(torch.isfinite(lam), lam, torch.zeros_like(lam)).float().reshape(H, W)
    lam[torch.from_numpy(rng.uniform(size=(H, W)) < 0.02).to(dev)] = 0.0
    return lam


def make_views(n, dev, seed=1):
    rng = np.random.default_rng(seed)
    bx = boxes()
    f = 0.9 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    views = []
    for k in range(n):
        C = np.array([rng.uniform(-250, 250), rng.uniform(-250, 250), rng.uniform(400, 600)])
        T = C * [1, 1, 0] if k % 2 == 0 else np.array([rng.uniform(-150, 150), rng.uniform(-150, 150), 0.0])
        E = look_at(C, T)
        depth = render(K, E, bx, dev, rng)
        views.append(mesh.MeshView(K, E, depth, torch.full((H, W), 0.9, dtype=torch.float32, device=dev)))
    return views


def torch_integrate(vol, grid, views, trunc, conf=mesh.DEFAULT_CONF):
    """The comparator: mesh.py's integration in fp64 torch over the allocated voxels, one view at a time."""
    bx, by, _ = grid.bricks
    b = vol["bricks"].long()
    dev = b.device
    l = torch.arange(512, device=dev)
    gi = ((b % bx) * 8)[:, None] + (l & 7)
    gj = (((b // bx) % by) * 8)[:, None] + ((l >> 3) & 7)
    gk = ((b // (bx * by)) * 8)[:, None] + (l >> 6)
    ex = (gi < grid.n[0]) & (gj < grid.n[1]) & (gk < grid.n[2])
    X = [grid.min[a] + (g.double() + 0.5) * grid.voxel for a, g in enumerate((gi, gj, gk))]
    s = torch.zeros(gi.shape, dtype=torch.float32, device=dev)
    n = torch.zeros(gi.shape, dtype=torch.int32, device=dev)
    for v in views:
        R, t, K = v.R.tolist(), v.t.tolist(), v.K.tolist()
        p = [R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r] for r in range(3)]
        q = [K[r][0] * p[0] + K[r][1] * p[1] + K[r][2] * p[2] for r in range(3)]
        px, py = torch.floor(q[0] / q[2] + 0.5), torch.floor(q[1] / q[2] + 0.5)
        ok = ex & (p[2] > 0) & (q[2] > 0) & (px >= 0) & (px <= v.W - 1) & (py >= 0) & (py <= v.H - 1)
        idx = torch.where(ok, py * v.W + px, torch.zeros_like(px)).long()
        D, c = v.depth.reshape(-1)[idx], v.confidence.reshape(-1)[idx]
        sdf = D.double() - p[2]
        ok = ok & torch.isfinite(D) & (D > 0) & (c.double() >= conf) & (sdf >= -trunc)
        s = torch.where(ok, s + torch.clamp(sdf / trunc, max=1.0).float(), s)
        n += ok.int()
    return s.reshape(-1, 8, 8, 8), n.reshape(-1, 8, 8, 8)


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


def run(views, voxel, iters):
    grid = mesh.MeshGrid(BORDER, voxel)
    trunc = 3 * voxel
    lib = mesh._lib.load()
    vol = mesh.tsdf_volume(views, grid)
    nb = int(vol["bricks"].shape[0])
    # allocation alone: mark + bricks, the same calls tsdf_volume makes
    g = grid.record()
    bx, by, bz = grid.bricks
    marks = torch.zeros(((bz + 2) * (by + 2) * (bx + 2),), dtype=torch.uint8, device="cuda")
    recs = mesh._records(views, "cuda")
    nbytes = int(lib.d3d_mesh_scan_scratch_bytes(grid.n_bricks))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    index = torch.empty((bz, by, bx), dtype=torch.int32, device="cuda")
    blist = torch.empty((grid.n_bricks,), dtype=torch.int32, device="cuda")
    nbd = torch.empty((1,), dtype=torch.int64, device="cuda")
    P = mesh._ptr

    def alloc():
        marks.zero_()
        mesh._lib.check(lib.d3d_mesh_mark(mesh.ctypes.byref(g), P(recs), len(views), W * H, mesh.DEFAULT_CONF, P(marks), mesh._stream()), "mark")
        mesh._lib.check(lib.d3d_mesh_bricks(mesh.ctypes.byref(g), P(marks), P(scratch), nbytes, P(index), P(blist), P(nbd), mesh._stream()),
                        "bricks")

    s = torch.zeros_like(vol["sum"])
    n = torch.zeros_like(vol["count"])

    def integ():
        s.zero_()
        n.zero_()
        mesh._lib.check(lib.d3d_mesh_integrate(mesh.ctypes.byref(g), P(vol["bricks"]), nb, P(recs), len(views), trunc, mesh.DEFAULT_CONF,
                                               P(s), P(n), mesh._stream()), "integrate")

    t_alloc = timed_ms(alloc, iters)
    t_int = timed_ms(integ, iters)
    t_ext = timed_ms(lambda: mesh.extract(vol, grid), iters)   # includes its three small device-to-host reads of the counts
    V, F = mesh.extract(vol, grid)
    obs = vol["count"] >= mesh.DEFAULT_MIN_VIEWS
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    ts, tn = torch_integrate(vol, grid, views, trunc)
    t1.record()
    torch.cuda.synchronize()
    same = bool(torch.equal(ts.view(torch.int32), vol["sum"].view(torch.int32)) and torch.equal(tn, vol["count"]))
    return {"views": len(views), "voxel_m": voxel, "grid": list(grid.n), "bricks_total": grid.n_bricks, "bricks_allocated": nb,
            "alloc_ms": round(t_alloc, 3), "integrate_ms": round(t_int, 3), "extract_ms": round(t_ext, 3),
            "torch_integrate_ms": round(t0.elapsed_time(t1), 1), "torch_same_bits": same, "vertices": int(V.shape[0]),
            "faces": int(F.shape[0]), "observed_voxels": int(obs.sum()),
            "views_per_observed_voxel": round(float(vol["count"][obs].double().mean()), 2) if bool(obs.any()) else 0.0}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--views", default="32,128")
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    a = ap.parse_args(argv)
    res = {"device": torch.cuda.get_device_name(0), "image": [W, H], "border": BORDER, "runs": []}
    for nv in (int(x) for x in a.views.split(",")):
        views = make_views(nv, "cuda")
        for voxel in (float(x) for x in a.voxels.split(",")):
            res["runs"].append(run(views, voxel, a.iters))
            print(json.dumps(res["runs"][-1]), file=sys.stderr)
        del views
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
