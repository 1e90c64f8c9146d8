"""The outlines (csrc/outlines.hip, deep3d_aerial_amd/outlines.py) on the three inputs of tools/objects_bench.py at --size cells
square: the label raster objects.segment makes of "scene" (the terrain bench's nDSM), "serpentine" (one winding band) and
"random" (density 0.59 under connectivity 4).  Per input: device-event ms (one warm-up, then --runs timed calls, each on its own
events: median, min, max) of objects.segment (the stage before this one, for scale) and of the whole outlines.label_outlines call
(its allocations and host reads included); then on preallocated buffers the phases count, edges, every round of the ranking and
emit (rings, place, emit), each with the bytes it has to move and that as a share of 8 TB/s: a round reads an edge's own state,
gathers its successor's and writes one (3 x 16 bytes an edge; 3 x 12 in the split form); n_edges, n_rings, n_vertices and rounds.
With --variant_library SO (a `make OUTLINES=split` build) the rounds of both builds take turns on buffers of their own and must
rank the edges alike.  The host part -- polygons() and geojson_bytes() -- is timed on the wall clock; the text is skipped above
--host_max_vertices.  The yardstick at --yardstick_size is the serial trace of tests/outlines_scene.py on the host and, where it
imports, skimage.measure.find_contours or scipy's binary label of the same raster (neither makes rings per object with holes).
What bounds the kernels is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/outlines_bench.py [--runs 5] [--size 10000] [--unit 0.1] [--inputs scene,serpentine,random] [--yardstick_size 1000]
        [--variant_library SO] [--host_max_vertices 3000000] [--out profiles/outlines_bench.json]"""
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

from deep3d_aerial_amd import _geom, _lib, objects, outlines  # noqa: E402
from bench_common import PEAK_BYTES_PER_S, bind, timed  # noqa: E402
from dtm_bench import stats  # noqa: E402  (the multiple-of-8-TB/s form)
from objects_bench import make_inputs  # noqa: E402


def rank(lib, state, E, st):
    """The rounds of the ranking, each on its own events: ([ms per round], index of the buffer that holds the result)."""
    P = _geom.ptr
    changed = torch.empty((1,), dtype=torch.int32, device="cuda")
    ms, k = [], 0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.d3d_outlines_rank(P(state[k & 1]), P(state[1 - (k & 1)]), E, k, P(changed), st), "rank")
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        k += 1
        if not int(changed[0]):
            return ms, k & 1


def ranked(state, E, split):
    """(m, dm) of a state buffer in either layout."""
    flat = state.view(-1)
    return (flat[:E], flat[E:2 * E]) if split else (state[:, 0], state[:, 1])


def measure(ndsm, grid, conn, runs, variant, host_max_vertices):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    H, W = ndsm.shape
    cells = H * W
    res = {"connectivity": conn}
    keep = {}
    res["objects_segment"] = stats(timed(lambda: keep.update(o=objects.segment(ndsm, grid, connectivity=conn)), runs), 8 * cells)
    label, table = keep.pop("o")
    info = {}
    res["label_outlines"] = stats(timed(lambda: keep.update(r=outlines.label_outlines(label, conn, info=info)), runs))
    rings = keep.pop("r")
    E, R, V = info["edges"], info["rings"], int(rings["vertices"].shape[0])
    res.update(n_objects=int(table["id"].shape[0]), n_edges=E, n_rings=R, n_vertices=V, rounds=info["rounds"])
    if E == 0:
        return res
    # the host part
    t0 = time.perf_counter()
    polys = outlines.polygons(rings, grid, conn)
    res["host_polygons_s"] = round(time.perf_counter() - t0, 3)
    if V <= host_max_vertices:
        t0 = time.perf_counter()
        data = outlines.geojson_bytes(polys, table)
        res["host_geojson_s"], res["geojson_bytes"] = round(time.perf_counter() - t0, 3), len(data)
        del data
    else:
        res["host_geojson_s"] = "skipped: %d vertices, more than --host_max_vertices" % V
    del polys, rings
    torch.cuda.empty_cache()
    # the phases on preallocated buffers
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    scratch, nbytes = _geom.scratch(lib.d3d_outlines_scratch_bytes, W, H, device="cuda")
    offset, counters, count = i32(H, W), torch.empty((2,), dtype=torch.int64, device="cuda"), torch.empty((2,), dtype=torch.int64, device="cuda")
    succ, key, ring_id, ordered, corner = (i32(E) for _ in range(5))
    state = [i32(E, 4), i32(E, 4)]
    ring_len, ring_edge, ring_object, vertices, ring_start = i32(R), i32(R), i32(R), i32(V, 2), i32(R + 1)
    res["count"] = stats(timed(lambda: _lib.check(lib.d3d_outlines_count(P(label), W, H, P(offset), P(scratch), nbytes, P(counters), st), "count"),
                               runs), 16 * cells)   # the labels read, the counts written, the scan's read and write
    edges_call = lambda L, s: _lib.check(L.d3d_outlines_edges(P(label), P(offset), conn, W, H, E, P(succ), P(key), P(s), st), "edges")
    res["edges"] = stats(timed(lambda: edges_call(lib, state[0]), runs), 8 * cells + 24 * E)
    per_round = []
    for _ in range(runs):
        edges_call(lib, state[0])
        ms, at = rank(lib, state, E, st)
        per_round.append(ms)
    per_round = np.array(per_round)
    res["rank"] = stats(per_round.sum(1).tolist(), 48 * E * per_round.shape[1])
    res["rank"]["rounds_ms_median"] = [round(float(v), 4) for v in np.median(per_round, 0)]
    res["rank"]["bytes_per_round"] = 48 * E
    res["rank"]["share_of_8TBps_per_round"] = [round(48 * E / PEAK_BYTES_PER_S * 1e3 / max(float(v), 1e-9), 4) for v in np.median(per_round, 0)]
    if variant:
        other = bind(variant)
        state2 = [i32(E, 4), i32(E, 4)]
        a_ms, b_ms = [], []
        for _ in range(runs):   # taking turns
            edges_call(lib, state[0])
            ms, at = rank(lib, state, E, st)
            a_ms.append(sum(ms))
            edges_call(other, state2[0])
            ms2, at2 = rank(other, state2, E, st)
            b_ms.append(sum(ms2))
        same = all(torch.equal(x, y) for x, y in zip(ranked(state[at], E, False), ranked(state2[at2], E, True))) and len(ms) == len(ms2)
        res["rank_variants"] = {"records": stats(a_ms, 48 * E * len(ms)), "split": stats(b_ms, 36 * E * len(ms2)),
                                "split_rounds_ms_last_run": [round(v, 4) for v in ms2], "variant_library": variant, "same_ranks": bool(same)}
        del state2
        edges_call(lib, state[0])
        _, at = rank(lib, state, E, st)

    def emit_call():
        _lib.check(lib.d3d_outlines_rings(P(state[at]), W, H, E, P(ring_id), P(scratch), nbytes, P(count[0:1]), st), "rings")
        _lib.check(lib.d3d_outlines_place(P(label), W, H, P(state[at]), P(succ), P(key), P(ring_id), E, R, P(ring_len), P(ring_edge),
                                          P(ring_object), P(ordered), P(corner), P(scratch), nbytes, P(count[1:2]), st), "place")
        _lib.check(lib.d3d_outlines_emit(P(ordered), P(corner), P(ring_edge), W, H, E, R, V, P(vertices), P(ring_start), st), "emit")

    res["emit"] = stats(timed(emit_call, runs), 92 * E + 8 * V)
    assert count.tolist() == [R, V]
    return res


def yardstick(ndsm, grid, conn):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import outlines_scene as S

    label, _ = objects.segment(ndsm, grid, connectivity=conn)
    info = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = outlines.label_outlines(label, conn, info=info)
    torch.cuda.synchronize()
    res = {"size": list(label.shape), "label_outlines_ms": round((time.perf_counter() - t0) * 1e3, 3), "edges": info["edges"], "rings": info["rings"]}
    host = label.cpu().numpy()
    t0 = time.perf_counter()
    rings = S.trace(host, conn)
    res["serial_trace_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    v, start, obj = S.arrays(rings)
    res["same_rings"] = bool(np.array_equal(got["vertices"].cpu().numpy(), v) and np.array_equal(got["ring_start"].cpu().numpy(), start)
                             and np.array_equal(got["ring_object"].cpu().numpy(), obj))
    try:
        from skimage import measure

        t0 = time.perf_counter()
        measure.find_contours((host > 0).astype(np.float64), 0.5)
        res["skimage_find_contours_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    except ImportError:
        res["skimage_find_contours_ms"] = "skimage does not import"
    try:
        from scipy import ndimage

        t0 = time.perf_counter()
        ndimage.label(host > 0)
        res["scipy_label_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    except ImportError:
        res["scipy_label_ms"] = "scipy does not import"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--unit", type=float, default=0.1)
    ap.add_argument("--inputs", default="scene,serpentine,random", help="which of the three inputs to measure")
    ap.add_argument("--yardstick_size", type=int, default=1000, help="0: no yardstick")
    ap.add_argument("--variant_library", default=None, metavar="SO", help="an OUTLINES=split build of the library whose ranking is timed beside this one")
    ap.add_argument("--host_max_vertices", type=int, default=3000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlines_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/outlines_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "peak_bytes_per_s": PEAK_BYTES_PER_S,
           "size": [a.size, a.size], "unit": a.unit, "runs": a.runs, "inputs": {}, "yardsticks": {}}
    wanted = a.inputs.split(",")
    if a.size > 0:
        grid, inputs = make_inputs(a.size, a.unit)
        if not set(wanted) <= set(inputs):
            ap.error("--inputs: a comma list of %s" % ", ".join(inputs))
        for name in list(inputs):
            ndsm, conn = inputs.pop(name)
            if name in wanted:
                res["inputs"][name] = measure(ndsm, grid, conn, a.runs, a.variant_library, a.host_max_vertices)
                print(json.dumps({name: res["inputs"][name]}), file=sys.stderr, flush=True)
            del ndsm
            torch.cuda.empty_cache()
    for name in (wanted if a.yardstick_size > 0 else []):
        g, small = make_inputs(a.yardstick_size, a.unit)
        res["yardsticks"][name] = yardstick(small[name][0], g, small[name][1])
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
