"""The object segmentation (csrc/objects.hip, deep3d_aerial_amd/objects.py) on three inputs of --size cells square at --unit world
units per cell: "scene", the nDSM of tools/dtm_bench.py's synthetic DSM through dsm_to_dtm; "serpentine", one winding band that
crosses every tile (every other row full, joined at alternating ends); "random", foreground at density 0.59 under connectivity 4
(the percolation threshold, where components are at their most ragged).  Per input: device-event ms (one warm-up, then --runs
timed calls, each on its own events: median, min, max) of the whole objects.segment call (its allocations and its host read
included) and of each entry point on preallocated buffers -- label (the tile, border and resolve kernels), roots, stats, relabel
-- each as a multiple of the floor, the nDSM read once and the int32 label written once (8 bytes per cell) at 8 TB/s; the
components, the objects and the border merge's hooks and repeated passes.  With --variant_library SO (a `make OBJECTS=plain`
build) the statistics pass of both builds runs on the same buffers, taking turns, and must give the same bits.  The yardsticks
run on the same kinds of input at --yardstick_size (the serpentine at --yardstick_serpentine, since its fixed point needs as
many rounds as the band is long): label propagation in torch (the index raster under a masked max_pool2d, iterated until nothing
changes), which must find as many components, and scipy.ndimage.label on the host where scipy imports.
What bounds the kernels is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

Under a kernel trace, --inputs NAME --yardstick_size 0 keeps one input's kernels apart from the others'.

    python tools/objects_bench.py [--runs 5] [--size 10000] [--unit 0.1] [--inputs scene,serpentine,random] [--yardstick_size 2000]
        [--yardstick_serpentine 256] [--variant_library SO] [--out profiles/objects_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deep3d_aerial_amd import _geom, _lib, dtm, objects  # noqa: E402
from deep3d_aerial_amd.dsm import DsmGrid  # noqa: E402
from bench_common import PEAK_BYTES_PER_S, bind, timed  # noqa: E402
from dtm_bench import make_dsm, stats  # noqa: E402  (the DSM of that tool, and its multiple-of-8-TB/s stats)

MAX_ROUNDS = 200000


def make_inputs(n, unit):
    """{name: (ndsm [n,n] fp32 on the GPU, connectivity)}"""
    grid = DsmGrid([0.0, n * unit, 0.0, n * unit], [unit, unit], size=(n, n))
    scene = dtm.dsm_to_dtm(make_dsm(n, unit), grid)[2]
    torch.cuda.empty_cache()
    band = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    band[::2] = 5.0
    band[1::4, n - 1] = 5.0
    band[3::4, 0] = 5.0
    gen = torch.Generator(device="cuda").manual_seed(1)
    random = torch.where(torch.rand((n, n), device="cuda", generator=gen) < 0.59, 5.0, 0.0).contiguous()
    return grid, {"scene": (scene, 8), "serpentine": (band, 8), "random": (random, 4)}


def measure(ndsm, grid, conn, runs, variant):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    H, W = ndsm.shape
    cells = H * W
    floor_bytes = 8 * cells
    res = {"connectivity": conn}
    info, state = {}, {}
    res["segment"] = stats(timed(lambda: state.update(o=objects.segment(ndsm, grid, connectivity=conn, info=info)), runs), floor_bytes)
    res.update(components=info["components"], objects=info["objects"], hooks=info["hooks"], repeated_passes=info["repeats"],
               foreground_share=round(float((ndsm >= 2.0).float().mean()), 4))
    state.clear()
    torch.cuda.empty_cache()
    need = objects.min_cells(grid)
    parent = torch.empty((H, W), dtype=torch.int32, device="cuda")
    label = torch.empty((H, W), dtype=torch.int32, device="cuda")
    count = torch.empty((2,), dtype=torch.int64, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_objects_scratch_bytes, W, H, device="cuda")
    res["label"] = stats(timed(lambda: _lib.check(lib.d3d_objects_label(P(ndsm), 2.0, None, conn, P(parent), W, H, None, st), "label"), runs),
                         floor_bytes)
    res["roots"] = stats(timed(lambda: _lib.check(lib.d3d_objects_roots(P(parent), W, H, P(scratch), nbytes, P(count[0:1]), st), "roots"),
                               runs), floor_bytes)
    n_roots = int(count[0])
    acc = torch.empty((max(n_roots, 1), objects.SLOTS), dtype=torch.int64, device="cuda")
    final_id = torch.empty((max(n_roots, 1),), dtype=torch.int32, device="cuda")

    def stats_call(L=lib, a=acc):
        _lib.check(L.d3d_objects_stats(P(ndsm), P(parent), W, H, P(scratch), nbytes, n_roots, P(a), st), "stats")

    res["stats"] = stats(timed(stats_call, runs), floor_bytes)
    if variant:
        other = bind(variant)
        acc2 = torch.empty_like(acc)
        a_ms, b_ms = [], []
        for _ in range(runs):   # taking turns
            a_ms += timed(stats_call, 1)
            b_ms += timed(lambda: stats_call(other, acc2), 1)
        res["stats_variants"] = {"run_reduction": stats(a_ms, floor_bytes), "one_set_per_cell": stats(b_ms, floor_bytes),
                                 "variant_library": variant, "same_bits": bool(torch.equal(acc, acc2))}
        del acc2
    res["relabel"] = stats(timed(lambda: _lib.check(lib.d3d_objects_relabel(P(parent), P(acc), n_roots, need, P(final_id), P(label), W, H,
                                                                            P(scratch), nbytes, P(count[1:2]), st), "relabel"), runs),
                           floor_bytes)
    return res


def propagate(mask, conn, max_rounds=MAX_ROUNDS):
    """(labels, rounds): the largest index + 1 of each component by masked max pooling to the fixed point (None past max_rounds)."""
    F = torch.nn.functional
    H, W = mask.shape
    lab = torch.where(mask, torch.arange(1, H * W + 1, device=mask.device, dtype=torch.float32).reshape(H, W), 0.0)[None, None]
    m = mask[None, None]
    rounds = 0
    while rounds < max_rounds:
        for _ in range(16):
            prev = lab
            if conn == 8:
                lab = F.max_pool2d(lab, 3, stride=1, padding=1)
            else:
                lab = torch.maximum(F.max_pool2d(lab, (3, 1), stride=1, padding=(1, 0)), F.max_pool2d(lab, (1, 3), stride=1, padding=(0, 1)))
            lab = torch.where(m, lab, 0.0)
            rounds += 1
        if torch.equal(lab, prev):
            return lab[0, 0], rounds
    return None, rounds


def yardsticks(ndsm, grid, conn):
    H, W = ndsm.shape
    assert H * W < 1 << 24   # the propagated indices are fp32
    mask = ndsm >= 2.0
    info = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parent = objects.label_components(mask, conn, info=info)
    torch.cuda.synchronize()
    res = {"size": [H, W], "label_components_ms": round((time.perf_counter() - t0) * 1e3, 3)}
    ours = int((parent == torch.arange(H * W, device="cuda", dtype=torch.int32).reshape(H, W)).sum())
    res["components"] = ours
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab, rounds = propagate(mask, conn)
    torch.cuda.synchronize()
    res["torch_propagation"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "rounds": rounds, "finished": lab is not None}
    if lab is not None:
        res["torch_propagation"]["same_components"] = int(torch.unique(lab[mask]).numel()) == ours
        res["torch_propagation"]["torch_over_hip"] = round(res["torch_propagation"]["ms"] / max(res["label_components_ms"], 1e-6), 1)
    try:
        from scipy import ndimage
    except ImportError:
        res["scipy_label"] = {"error": "scipy does not import"}
        return res
    host = mask.cpu().numpy()
    t0 = time.perf_counter()
    _, n = ndimage.label(host, structure=np.ones((3, 3), int) if conn == 8 else None)
    res["scipy_label"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "same_components": int(n) == ours}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--unit", type=float, default=0.1)
    ap.add_argument("--inputs", default="scene,serpentine,random", help="which of the three inputs to measure")
    ap.add_argument("--yardstick_size", type=int, default=2000, help="0: no yardsticks")
    ap.add_argument("--yardstick_serpentine", type=int, default=256)
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="an OBJECTS=plain build of the library whose statistics pass is timed beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/objects_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "size": [a.size, a.size], "unit": a.unit,
           "runs": a.runs, "tile": objects.TILE, "inputs": {}, "yardsticks": {}}
    grid, inputs = make_inputs(a.size, a.unit)
    wanted = a.inputs.split(",")
    if not set(wanted) <= set(inputs):
        ap.error("--inputs: a comma list of %s" % ", ".join(inputs))
    for name in list(inputs):
        ndsm, conn = inputs.pop(name)
        if name not in wanted:
            continue
        res["inputs"][name] = measure(ndsm, grid, conn, a.runs, a.variant_library)
        print(json.dumps({name: res["inputs"][name]}), file=sys.stderr, flush=True)
        del ndsm
        torch.cuda.empty_cache()
    for name in (wanted if a.yardstick_size > 0 else []):
        n = a.yardstick_serpentine if name == "serpentine" else a.yardstick_size
        g, small = make_inputs(n, a.unit)
        ndsm, conn = small[name]
        res["yardsticks"][name] = yardsticks(ndsm, g, conn)
        print(json.dumps({name: res["yardsticks"][name]}), file=sys.stderr, flush=True)
    res["bound"] = "unconfirmed (no kernel trace or counters in this run)"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
