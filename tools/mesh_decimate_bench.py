"""The decimation kernels (csrc/mesh_decimate.hip) at survey size: the 600 x 600 m scene of tools/mesh_bench.py (ground and 120 box
buildings, 32 views of 2752 x 1856) meshed at 0.5 m (and 0.25 m) voxels, after clean(min_faces=20, smooth=1).  For the ratios 0.5,
0.25 and 0.1: rounds, faces out, stalled or not, and the device-event time of the whole mesh.decimate (one warm-up, median of 5);
for the first round of each mesh the time of every pass (adjacency, incidence, quadrics, and the rest of the round: edges,
candidates, select, claim, apply, faces, compact).  No torch same-bits comparator is timed here: the bit-level reference is the
numpy restatement of tests/test_mesh_decimate.py.  Prints one JSON line (and writes --out).

    python tools/mesh_decimate_bench.py [--voxels 0.5] [--views 32] [--ratios 0.5,0.25,0.1] [--out profiles/mesh_decimate_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mesh_bench as MB  # noqa: E402
import mesh_clean_bench as CB  # noqa: E402
from deep3d_aerial_amd import mesh  # noqa: E402


def run(voxel, views, ratios, reps):
    V, F = mesh.clean(*mesh.depth_to_mesh(views, mesh.MeshGrid(MB.BORDER, voxel)), min_faces=20, smooth=1)
    n, m = int(V.shape[0]), int(F.shape[0])
    inc = mesh.face_incidence(F, n)
    first = {"adjacency_ms": CB.median_ms(lambda: mesh.adjacency(F, n), reps), "incidence_ms": CB.median_ms(lambda: mesh.face_incidence(F, n), reps),
             "quadrics_ms": CB.median_ms(lambda: mesh.vertex_quadrics(V, F, inc), reps),
             "whole_round_ms": CB.median_ms(lambda: mesh.decimate_round(V, F, m // 2), reps)}
    first["rest_of_round_ms"] = first["whole_round_ms"] - first["adjacency_ms"] - first["incidence_ms"] - first["quadrics_ms"]
    res = {"voxel": voxel, "vertices": n, "triangles": m, "first_round": first, "ratios": []}
    for r in ratios:
        info = {}
        mesh.decimate(V, F, ratio=r, info=info)
        res["ratios"].append({"ratio": r, "target_faces": info["target_faces"], "faces_out": info["faces_out"], "vertices_out": info["vertices_out"],
                              "rounds": info["rounds"], "stalled": info["stalled"], "hit_max_rounds": info["hit_max_rounds"],
                              "first_round_collapses": info["collapses"][0] if info["collapses"] else 0,
                              "decimate_ms": CB.median_ms(lambda: mesh.decimate(V, F, ratio=r), reps)})
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--voxels", default="0.5")
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--ratios", default="0.5,0.25,0.1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.cuda.set_device(0)
    views = CB.make_views(a.views, 0, "cuda")
    out = {"tool": "mesh_decimate_bench", "views": a.views, "device": torch.cuda.get_device_name(0),
           "runs": [run(float(v), views, [float(r) for r in a.ratios.split(",")], a.reps) for v in a.voxels.split(",")]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
