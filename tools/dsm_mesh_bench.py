"""The DSM-from-mesh kernels (csrc/dsm.hip dsm_tri_*) on the synthetic scene of tools/mesh_bench.py: the meshes of 32 views at
0.5 m and 0.25 m voxels rasterised at 0.2 m over the scene (3000 x 3000), plus two stress cases on the same raster -- the mesh
at 10 m voxels (big triangles: the list kernel) and two triangles that span the raster.  Per case: device-event ms of the
d3d_dsm_from_mesh call (scratch allocated once; one warm-up, then --runs timed calls, each on its own events: median, min, max),
triangles/s, the bytes the call must move (about 48 B per triangle -- indices, three vertex gathers, the big-list entry --
plus 12 B per cell: clear, atomics, finalize) against the 8 TB/s HBM peak, which is an estimate and not a measurement, and
the share of triangles on the big list.  The comparator is the same semantics written in fp64 torch (this tool only), timed
once; both must give the same raster.  What bounds the kernels is not measured here.  Prints one JSON line (and writes --out).

    python tools/dsm_mesh_bench.py [--runs 5] [--voxels 0.5,0.25] [--out profiles/dsm_mesh_bench.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mesh_bench  # noqa: E402
from deep3d_aerial_amd import _lib, dsm, mesh  # noqa: E402

HBM_PEAK = 8.0e12
UNIT = 0.2


def keys64(z):
    """dsm_key of fp32 values as int64 (order-preserving, IEEE total order)."""
    u = z.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def torch_mesh_dsm(V, F, grid, chunk=1 << 25):
    """dsm.py's mesh semantics in fp64 torch: per (triangle, centre of its range) pair, in groups of at most `chunk` pairs."""
    dev = V.device
    F = F.long()
    P = V[F]                                                                   # [m,3,3] fp32
    P = P[torch.isfinite(P).all(2).all(1)]
    for i, j in ((0, 1), (1, 2), (0, 1)):                                     # lexicographic (x, y, z), total order per component
        kp, kq = keys64(P[:, i]), keys64(P[:, j])
        less = (kq[:, 0] < kp[:, 0]) | ((kq[:, 0] == kp[:, 0]) & ((kq[:, 1] < kp[:, 1]) | ((kq[:, 1] == kp[:, 1]) & (kq[:, 2] < kp[:, 2]))))
        a, b = P[:, i].clone(), P[:, j].clone()
        P[:, i] = torch.where(less[:, None], b, a)
        P[:, j] = torch.where(less[:, None], a, b)

    def edge(p, q):
        fwd = (p[:, 0] < q[:, 0]) | ((p[:, 0] == q[:, 0]) & (p[:, 1] <= q[:, 1]))
        u = torch.where(fwd[:, None], p, q).double()
        v = torch.where(fwd[:, None], q, p).double()
        return [u[:, 0], u[:, 1], v[:, 0] - u[:, 0], v[:, 1] - u[:, 1], torch.where(fwd, 1.0, -1.0).double()]

    a, b, c = P[:, 0], P[:, 1], P[:, 2]
    E = [edge(b, c), edge(c, a), edge(a, b)]
    ox, oy, ex, ey, s = E[2]
    D = s * (ex * (c[:, 1].double() - oy) - ey * (c[:, 0].double() - ox))
    keep = (D != 0) & torch.isfinite(D)
    sigma = torch.where(D > 0, 1.0, -1.0).double()
    E = [[e[0][keep], e[1][keep], e[2][keep], e[3][keep], (e[4] * sigma)[keep]] for e in E]
    P = P[keep]
    z = P[:, :, 2].double()
    j0 = torch.clamp(torch.floor((P[:, :, 0].amin(1).double() - grid.x_min) / grid.unit[0]) - 1, min=0)
    j1 = torch.clamp(torch.floor((P[:, :, 0].amax(1).double() - grid.x_min) / grid.unit[0]) + 1, max=grid.width - 1)
    i0 = torch.clamp(torch.floor((grid.y_max - P[:, :, 1].amax(1).double()) / grid.unit[1]) - 1, min=0)
    i1 = torch.clamp(torch.floor((grid.y_max - P[:, :, 1].amin(1).double()) / grid.unit[1]) + 1, max=grid.height - 1)
    ok = (j0 <= j1) & (i0 <= i1)
    j0, i0 = torch.where(ok, j0, 0).long(), torch.where(ok, i0, 0).long()
    nj = torch.where(ok, j1.long() - j0 + 1, 0)
    n = nj * torch.where(ok, i1.long() - i0 + 1, 0)
    csum = torch.cumsum(n, 0)
    keymax = torch.zeros(grid.width * grid.height, dtype=torch.int64, device=dev)
    total, start_pair, t0 = int(csum[-1]) if len(n) else 0, 0, 0
    while start_pair < total:
        t1 = int(torch.searchsorted(csum, start_pair + chunk, right=True))
        t1 = max(t1, t0 + 1)
        cnt = n[t0:t1]
        tri = torch.repeat_interleave(torch.arange(t0, t1, device=dev), cnt)
        local = torch.arange(int(cnt.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        i = i0[tri] + local // nj[tri]
        j = j0[tri] + local % nj[tri]
        px = grid.x_min + (j.double() + 0.5) * grid.unit[0]
        py = grid.y_max - (i.double() + 0.5) * grid.unit[1]
        w = [e[4][tri] * (e[2][tri] * (py - e[1][tri]) - e[3][tri] * (px - e[0][tri])) for e in E]
        W = (w[0] + w[1]) + w[2]
        cov = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (W > 0)
        zz = (((w[0] * z[tri, 0] + w[1] * z[tri, 1]) + w[2] * z[tri, 2]) / torch.where(cov, W, 1.0)).float()
        cov &= (zz.double() >= grid.z_min) & (zz.double() <= grid.z_max)
        keymax.scatter_reduce_(0, (i * grid.width + j)[cov], keys64(zz[cov]), "amax")
        start_pair = int(csum[t1 - 1])
        t0 = t1
    k = keymax.reshape(grid.shape)
    bits = torch.where(k >= 0x80000000, k & 0x7FFFFFFF, (~k) & 0xFFFFFFFF)
    h = torch.where(bits >= 0x80000000, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)
    return torch.where(k == 0, torch.full_like(h, float("nan")), h)


def big_share(V, F, grid):
    P = V[F.long()]
    fin = torch.isfinite(P).all(2).all(1)
    x_lo, x_hi = P[:, :, 0].amin(1).double(), P[:, :, 0].amax(1).double()
    y_lo, y_hi = P[:, :, 1].amin(1).double(), P[:, :, 1].amax(1).double()
    nj = torch.clamp(torch.floor((x_hi - grid.x_min) / grid.unit[0]) + 1, max=grid.width - 1) - \
        torch.clamp(torch.floor((x_lo - grid.x_min) / grid.unit[0]) - 1, min=0) + 1
    ni = torch.clamp(torch.floor((grid.y_max - y_lo) / grid.unit[1]) + 1, max=grid.height - 1) - \
        torch.clamp(torch.floor((grid.y_max - y_hi) / grid.unit[1]) - 1, min=0) + 1
    big = fin & (nj > 0) & (ni > 0) & (nj * ni > dsm.DSM_TRI_SMALL)
    return float(big.double().mean()) if len(big) else 0.0


def run(name, V, F, grid, runs):
    lib = _lib.load()
    H, W = grid.shape
    nf, nv = int(F.shape[0]), int(V.shape[0])
    nbytes = int(lib.d3d_dsm_mesh_scratch_bytes(nf, W, H))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    height = torch.empty((H, W), dtype=torch.float32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        _lib.check(lib.d3d_dsm_from_mesh(P(V), nv, P(F), nf, grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], grid.z_min, grid.z_max,
                                         W, H, P(scratch), nbytes, P(height), dsm._stream()), "d3d_dsm_from_mesh")

    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    got = height.clone()
    same_op = bool(torch.equal(dsm.mesh_to_dsm(V, F, grid).view(torch.int32), got.view(torch.int32)))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    want = torch_mesh_dsm(V, F, grid)
    b.record()
    torch.cuda.synchronize()
    same = bool(torch.equal(want.view(torch.int32), got.view(torch.int32)))
    med = float(np.median(ms))
    est = 48.0 * nf + 12.0 * W * H
    return {"case": name, "triangles": nf, "vertices": nv, "raster": [W, H], "big_share": round(big_share(V, F, grid), 5),
            "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "runs": runs,
            "triangles_per_s": round(nf / (med * 1e-3), 1) if med > 0 else None, "est_bytes": int(est),
            "est_ms_at_hbm_peak": round(est / HBM_PEAK * 1e3, 4), "filled_cells": int(torch.isfinite(got).sum()),
            "torch_ms": round(a.elapsed_time(b), 1), "torch_same_bits": same, "operator_same_bits": same_op,
            "bound": "unconfirmed (no kernel trace or counters in this run)"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsm_mesh_bench.json"))
    a = ap.parse_args(argv)
    border = mesh_bench.BORDER
    grid = dsm.DsmGrid(border[:4], [UNIT, UNIT])
    res = {"device": torch.cuda.get_device_name(0), "border": border, "unit": UNIT, "hbm_peak_Bps": HBM_PEAK, "views": a.views, "runs": []}
    views = mesh_bench.make_views(a.views, "cuda")
    for voxel in [float(x) for x in a.voxels.split(",")] + [10.0]:
        V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
        torch.cuda.synchronize()
        res["runs"].append(dict(run("mesh_%gm" % voxel, V.contiguous(), F.contiguous(), grid, a.runs), voxel_m=voxel))
        print(json.dumps(res["runs"][-1]), file=sys.stderr)
        del V, F
        torch.cuda.empty_cache()
    del views
    x0, x1, y0, y1 = border[0] - 1.0, border[1] + 1.0, border[2] - 1.0, border[3] + 1.0
    V = torch.tensor([[x0, y0, 10.0], [x1, y0, 30.0], [x1, y1, 50.0], [x0, y1, 20.0]], dtype=torch.float32, device="cuda")
    F = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device="cuda")
    res["runs"].append(run("two_triangles_over_the_raster", V, F, grid, a.runs))
    print(json.dumps(res["runs"][-1]), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
