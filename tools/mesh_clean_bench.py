"""The mesh cleaning kernels (csrc/mesh_clean.hip) at survey size: the 600 x 600 m scene of tools/mesh_bench.py (ground and 120
box buildings, 32 views of 2752 x 1856) plus a few hundred floating boxes of 0.5-2 m ray-cast into every view like the
buildings, meshed at 0.5 m and 0.25 m voxels.  Device-event times (median of 5 after a warm-up) of the passes: components
(hooking + pointer jumping, the host reading one flag per round), removal (components + stats + filter + compact), adjacency of
the kept mesh, one smoothing iteration, and the full clean (removal, then one smoothing iteration); the component rounds and the
faces removed.  The comparator is the same removal and smoothing in torch (scatter-min labels, sort / unique adjacency, column
by column sums); both must give the same bits.  Bytes per pass are an estimate from the array sizes, not a measurement.
Prints one JSON line (and writes --out).

    python tools/mesh_clean_bench.py [--voxels 0.5,0.25] [--views 32] [--floaters 300] [--out profiles/mesh_clean_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mesh_bench as MB  # noqa: E402
from deep3d_aerial_amd import mesh  # noqa: E402

MIN_FACES, SPURIOUS = 20, 20.0   # the reference's fRemoveSpurious default, and a face floor


def floaters(seed=7, n=300):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(-280, 280, 2)
        s = rng.uniform(0.5, 2.0, 3)
        z0 = rng.uniform(100, 120)   # above every building (at most 90 m)
        out.append((cx - s[0] / 2, cx + s[0] / 2, cy - s[1] / 2, cy + s[1] / 2, z0, z0 + s[2]))
    return out


def render(K, E, bx, dev, rng):
    """Depth [H,W] of ground z = 0 and boxes (x0, x1, y0, y1, z0, z1), ray-cast in fp64 torch; 2 % holes."""
    W, H = MB.W, MB.H
    K64, E64 = torch.tensor(K, dtype=torch.float64, device=dev), torch.tensor(E, dtype=torch.float64, device=dev)
    R, t = E64[:3, :3], E64[:3, 3]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dc = torch.linalg.inv(K64) @ torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64, device=dev)])
    d = (R.T @ dc).T
    C = -R.T @ t
    lam = torch.where(d[:, 2] < 0, -C[2] / d[:, 2], torch.full_like(d[:, 2], math.inf))
    for x0, x1, y0, y1, z0, z1 in bx:
        lo = torch.tensor([x0, y0, z0], dtype=torch.float64, device=dev)
        hi = torch.tensor([x1, y1, z1], dtype=torch.float64, device=dev)
        t0, t1 = (lo - C) / d, (hi - C) / d
        tn = torch.minimum(t0, t1).nan_to_num(-math.inf).amax(1)
        tf = torch.maximum(t0, t1).nan_to_num(math.inf).amin(1)
        lam = torch.where((tn <= tf) & (tn > 0), torch.minimum(lam, tn), lam)
    lam = torch.where(torch.isfinite(lam), lam, torch.zeros_like(lam)).float().reshape(H, W)
    lam[torch.from_numpy(rng.uniform(size=(H, W)) < 0.02).to(dev)] = 0.0
    return lam


def make_views(n, n_floaters, dev, seed=1):
    rng = np.random.default_rng(seed)
    bx = [(x0, x1, y0, y1, 0.0, z1) for x0, x1, y0, y1, z1 in MB.boxes()] + floaters(n=n_floaters)
    W, H = MB.W, MB.H
    f = 0.9 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    views = []
    for k in range(n):
        C = np.array([rng.uniform(-250, 250), rng.uniform(-250, 250), rng.uniform(400, 600)])
        T = C * [1, 1, 0] if k % 2 == 0 else np.array([rng.uniform(-150, 150), rng.uniform(-150, 150), 0.0])
        E = MB.look_at(C, T)
        views.append(mesh.MeshView(K, E, render(K, E, bx, dev, rng), torch.full((H, W), 0.9, dtype=torch.float32, device=dev)))
    return views


# ----------------------------------------------------------------------------------------
# the torch comparator
# ----------------------------------------------------------------------------------------
def torch_labels(faces, n):
    f = faces.long()
    parent = torch.arange(n, device=faces.device)
    while True:
        p = parent[f]
        lo = p.min(1).values
        new = parent.clone().scatter_reduce_(0, p.reshape(-1), lo.repeat_interleave(3), "amin")
        while True:
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        if torch.equal(new, parent):
            return parent
        parent = new


def torch_remove(vertices, faces, min_faces, spurious):
    n = vertices.shape[0]
    f = faces.long()
    label = torch_labels(faces, n)
    r = label[f[:, 0]]
    count = torch.bincount(r, minlength=n)
    lo = torch.full((n, 3), math.inf, device=vertices.device).scatter_reduce_(0, label[:, None].expand(-1, 3), vertices, "amin")
    hi = torch.full((n, 3), -math.inf, device=vertices.device).scatter_reduce_(0, label[:, None].expand(-1, 3), vertices, "amax")
    d = hi.double() - lo.double()
    diag = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    used = torch.zeros(n, dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1)] = True
    g = vertices[used].max(0).values.double() - vertices[used].min(0).values.double()
    gdiag = torch.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    gone = torch.zeros(f.shape[0], dtype=torch.bool, device=f.device)
    if min_faces > 0:
        gone |= count[r] < min_faces
    if spurious > 0:
        gone |= diag[r] < gdiag / spurious
    kf = f[~gone]
    keep = torch.zeros(n, dtype=torch.bool, device=f.device)
    keep[kf.reshape(-1)] = True
    remap = torch.cumsum(keep.long(), 0) - 1
    return vertices[keep], remap[kf].int(), int(gone.sum())


def torch_smooth(vertices, faces, lam):
    n = vertices.shape[0]
    f = faces.long()
    p = torch.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1)
    lo, hi = p.min(2).values, p.max(2).values
    ok = lo != hi
    ok[:, 1] &= ~((lo[:, 1] == lo[:, 0]) & (hi[:, 1] == hi[:, 0]))
    ok[:, 2] &= ~(((lo[:, 2] == lo[:, 0]) & (hi[:, 2] == hi[:, 0])) | ((lo[:, 2] == lo[:, 1]) & (hi[:, 2] == hi[:, 1])))
    key, mult = torch.unique(lo[ok] * n + hi[ok], return_counts=True)
    a, b = key // n, key % n
    src, dst, m2 = torch.cat([a, b]), torch.cat([b, a]), torch.cat([mult, mult])
    order = torch.argsort(src * n + dst)
    src, dst, m2 = src[order], dst[order], m2[order]
    deg = torch.bincount(src, minlength=n)
    fixed = (deg == 0)
    fixed[src[m2 != 2]] = True
    start = torch.cumsum(deg, 0) - deg
    col = torch.arange(src.shape[0], device=f.device) - start[src]
    width = int(deg.max())
    s = torch.zeros_like(vertices)
    for k in range(width):
        sel = col == k
        s[src[sel]] = s[src[sel]] + vertices[dst[sel]]
    mean = s / deg.float()[:, None]
    out = vertices + (mean - vertices) * float(np.float32(lam))
    return torch.where(fixed[:, None], vertices, out)


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def run(voxel, views, grid_border):
    grid = mesh.MeshGrid(grid_border, voxel)
    V, F = mesh.depth_to_mesh(views, grid)
    n, m = int(V.shape[0]), int(F.shape[0])
    valence = torch.bincount(mesh.adjacency(F, n)[0].diff().clamp(max=64).long(), minlength=65)[:65].tolist()
    info = {}
    Vr, Fr = mesh.remove_components(V, F, MIN_FACES, SPURIOUS, info=info)
    csr = mesh.adjacency(Fr, Vr.shape[0])
    Vs = mesh.smooth_vertices(Vr, Fr, 1, csr=csr)
    Vc, Fc = mesh.clean(V, F, MIN_FACES, SPURIOUS, 1)
    tv, tf, removed = torch_remove(V, F, MIN_FACES, SPURIOUS)
    ts = torch_smooth(tv, tf, mesh.DEFAULT_SMOOTH_LAMBDA)
    same = (torch.equal(Vr.view(torch.int32), tv.view(torch.int32)) and torch.equal(Fr, tf) and torch.equal(Vs.view(torch.int32), ts.view(torch.int32))
            and torch.equal(Vc.view(torch.int32), ts.view(torch.int32)) and torch.equal(Fc, tf))
    nk, mk = int(Vr.shape[0]), int(Fr.shape[0])
    res = {
        "voxel": voxel, "vertices": n, "triangles": m, "kept_vertices": nk, "kept_triangles": mk, "faces_removed": info["faces_removed"],
        "torch_faces_removed": removed, "component_rounds": info["rounds"], "same_bits_as_torch": bool(same),
        "valence_histogram_0_to_64": valence,
        "components_ms": median_ms(lambda: mesh.components(F, n)),
        "removal_ms": median_ms(lambda: mesh.remove_components(V, F, MIN_FACES, SPURIOUS)),
        "adjacency_ms": median_ms(lambda: mesh.adjacency(Fr, nk)),
        "smooth_1_iteration_ms": median_ms(lambda: mesh.smooth_vertices(Vr, Fr, 1, csr=csr)),
        "full_clean_ms": median_ms(lambda: mesh.clean(V, F, MIN_FACES, SPURIOUS, 1)),
        "torch_comparator_ms": median_ms(lambda: torch_smooth(*torch_remove(V, F, MIN_FACES, SPURIOUS)[:2], 0.5), reps=1),
        # estimates from the array sizes (not measured): bytes each pass reads and writes once, atomics as a read and a write
        "est_bytes": {"components_per_round": 12 * m + 3 * 4 * m + 2 * 4 * n * 2, "stats": 12 * m + 12 * m + 12 * n + 4 * n + 24 * n * 2,
                      "filter_and_compact": 12 * m * 3 + 4 * m * 3 + 12 * n * 2 + 4 * n * 3,
                      "adjacency": 12 * mk * 2 + 4 * 6 * mk * 5 + 4 * nk * 8 + 8 * nk, "smooth_1": 12 * nk * 2 + 8 * nk + 4 * 6 * mk + 12 * 6 * mk},
    }
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--floaters", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.cuda.set_device(0)
    views = make_views(a.views, a.floaters, "cuda")
    out = {"tool": "mesh_clean_bench", "views": a.views, "floaters": a.floaters, "min_faces": MIN_FACES, "spurious": SPURIOUS,
           "device": torch.cuda.get_device_name(0), "runs": [run(float(v), views, MB.BORDER) for v in a.voxels.split(",")]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
