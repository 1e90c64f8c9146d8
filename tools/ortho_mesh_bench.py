"""The orthophoto-of-the-textured-mesh kernels (csrc/ortho_mesh.hip om_*) on the scenes of tools/dsm_mesh_bench.py: the meshes of
32 views at 0.5 m and 0.25 m voxels, the mesh at 10 m voxels (big triangles: the list kernel) and two triangles that span the
raster, rendered at 0.2 m (3000 x 3000) and at 0.1 m (6000 x 6000).  The meshes are textured from the same views with the
synthetic images of tools/texture_bench.py (select, layout, fill, texcoords); the two triangles get a page of noise laid over
the raster.  Per case and raster: device-event ms of the d3d_ortho_from_mesh call (scratch allocated once; one warm-up, then
--runs timed calls, each on its own events: median, min, max), the same for d3d_dsm_from_mesh on the same mesh and grid -- the
bare rasteriser, the code path the mesh DSM had before this stage -- and their ratio: what the colour costs over the coverage.
The ratio is reported, not pinned.  The height must be the DSM's bit for bit.  What bounds the kernels is not measured here: no
kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/ortho_mesh_bench.py [--runs 5] [--voxels 0.5,0.25] [--units 0.2,0.1] [--out profiles/ortho_mesh_bench.json]"""
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
import texture_bench  # noqa: E402
from bench_common import timed  # noqa: E402
from deep3d_aerial_amd import _lib, dsm, mesh, ortho_mesh, texture  # noqa: E402


def textured(V, F, ov):
    """(texcoord, texnumber, atlas, page_row, pages, charts) of the mesh textured from the views: texture.texture_mesh's passes,
    the atlas kept on the device."""
    key = texture.select_faces(V, F, ov)
    chart, labels, _, packing, table = texture.layout(V, F, key, ov)
    atlas = texture.finish_pages(texture.fill_pages(table, packing, ov, texture.new_atlas(packing, "cuda")))
    tc, tn = texture.texcoords(V, F, key, chart, table, packing, ov)
    return tc, tn, atlas, torch.from_numpy(packing.page_row).cuda(), packing.n_pages, int(labels.shape[0])


def run(name, V, F, tc, tn, atlas, page_row, grid, runs, z_down=False):
    lib = _lib.load()
    H, W = grid.shape
    nf, nv = int(F.shape[0]), int(V.shape[0])
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nbytes = int(lib.d3d_ortho_mesh_scratch_bytes(nf, W, H))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    height = torch.empty((H, W), dtype=torch.float32, device="cuda")
    n_pages, pw = int(page_row.shape[0]) - 1, int(atlas.shape[1])

    def ortho_call():
        _lib.check(lib.d3d_ortho_from_mesh(P(V), nv, P(F), nf, P(tc), P(tn), P(atlas), P(page_row), n_pages, pw, grid.x_min, grid.y_max,
                                           grid.unit[0], grid.unit[1], grid.z_min, grid.z_max, W, H, 1 if z_down else 0, P(scratch), nbytes,
                                           P(rgba), P(height), dsm._stream()), "d3d_ortho_from_mesh")

    ms = timed(ortho_call, runs)
    dbytes = int(lib.d3d_dsm_mesh_scratch_bytes(nf, W, H))
    dscratch = torch.empty((dbytes,), dtype=torch.uint8, device="cuda")
    dheight = torch.empty((H, W), dtype=torch.float32, device="cuda")

    def dsm_call():
        _lib.check(lib.d3d_dsm_from_mesh(P(V), nv, P(F), nf, grid.x_min, grid.y_max, grid.unit[0], grid.unit[1], grid.z_min, grid.z_max,
                                         W, H, P(dscratch), dbytes, P(dheight), dsm._stream()), "d3d_dsm_from_mesh")

    dms = timed(dsm_call, runs)
    same = bool(torch.equal(height.view(torch.int32), dheight.view(torch.int32))) if not z_down else None
    op = ortho_mesh.mesh_to_ortho(V, F, tc, tn, atlas, page_row, grid, z_down)
    same_op = bool(torch.equal(op[0], rgba) and torch.equal(op[1].view(torch.int32), height.view(torch.int32)))
    s = ortho_mesh.summary(rgba, height)
    med, dmed = float(np.median(ms)), float(np.median(dms))
    return {"case": name, "triangles": nf, "vertices": nv, "raster": [W, H], "unit": grid.unit[0], "pages": n_pages, "page_width": pw,
            "atlas_rows": int(atlas.shape[0]), "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "dsm_ms_median": round(dmed, 4), "dsm_ms_min": round(min(dms), 4), "dsm_ms_max": round(max(dms), 4),
            "ratio_to_dsm": round(med / dmed, 3) if dmed > 0 else None, "runs": runs,
            "triangles_per_s": round(nf / (med * 1e-3), 1) if med > 0 else None, "coloured": s["coloured"], "untextured": s["untextured"],
            "empty": s["empty"], "height_is_the_dsm": same, "operator_same_bits": same_op,
            "bound": "unconfirmed (no kernel trace or counters in this run)"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--voxels", default="0.5,0.25")
    ap.add_argument("--units", default="0.2,0.1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ortho_mesh_bench.json"))
    a = ap.parse_args(argv)
    border = mesh_bench.BORDER
    grids = [dsm.DsmGrid(border[:4], [u, u]) for u in (float(x) for x in a.units.split(","))]
    res = {"device": torch.cuda.get_device_name(0), "border": border, "units": [g.unit[0] for g in grids], "views": a.views, "runs": []}
    views = mesh_bench.make_views(a.views, "cuda")
    ov = texture_bench.ortho_views(views)
    for voxel in [float(x) for x in a.voxels.split(",")] + [10.0]:
        V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
        V, F = V.contiguous(), F.contiguous()
        tc, tn, atlas, page_row, _, n_charts = textured(V, F, ov)
        torch.cuda.synchronize()
        for g in grids:
            res["runs"].append(dict(run("mesh_%gm" % voxel, V, F, tc, tn, atlas, page_row, g, a.runs), voxel_m=voxel, charts=n_charts))
            print(json.dumps(res["runs"][-1]), file=sys.stderr)
        del V, F, tc, tn, atlas
        torch.cuda.empty_cache()
    del views, ov
    torch.cuda.empty_cache()
    x0, x1, y0, y1 = border[0] - 1.0, border[1] + 1.0, border[2] - 1.0, border[3] + 1.0
    V = torch.tensor([[x0, y0, 10.0], [x1, y0, 30.0], [x1, y1, 50.0], [x0, y1, 20.0]], dtype=torch.float32, device="cuda")
    F = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device="cuda")
    corner = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=torch.float32, device="cuda")
    tc = corner[F.long()].reshape(2, 6).contiguous()                          # the page laid over the quad
    tn = torch.zeros(2, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    atlas = torch.randint(-(1 << 31), (1 << 31) - 1, (4096, 4096), dtype=torch.int32, device="cuda", generator=gen)
    page_row = torch.tensor([0, 4096], dtype=torch.int64, device="cuda")
    for g in grids:
        res["runs"].append(run("two_triangles_over_the_raster", V, F, tc, tn, atlas, page_row, g, a.runs))
        print(json.dumps(res["runs"][-1]), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
