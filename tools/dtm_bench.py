"""The terrain filter (csrc/dtm.hip, deep3d_aerial_amd/dtm.py) on a synthetic DSM: a smooth terrain with box buildings, noise on a
1/64 grid and a share of empty cells, --size cells square at --unit world units per cell.  Per radius of --radii: device-event ms
of one opening (d3d_dtm_open on preallocated buffers; one warm-up, then --runs timed calls, each on its own events: median, min,
max), the bytes an opening must move (the raster read once and written once: 8 bytes per cell) as a time at 8 TB/s and the
measured time as a multiple of that, and the bytes this implementation moves (20 raster passes: five per running-extreme pass,
four passes).  The yardstick is what a user writes without this stage, in the same tool: the same opening with
torch.nn.functional.max_pool2d, stride 1, on tensors padded with +-inf (erosion as the negated maximum of the negation), a row
pass and a column pass per half, which must give the same values (NaN-free input: max_pool2d has no empty cell).  Then the opening
of every level of the default filter on that raster, and the whole dsm_to_dtm call (its allocations included).
What bounds the kernels is not measured here: no kernel trace and no counters are taken.  Prints one JSON line (and writes --out).

    python tools/dtm_bench.py [--runs 5] [--size 10000] [--unit 0.1] [--radii 1,16,128,1024] [--out profiles/dtm_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deep3d_aerial_amd import _geom, _lib, dtm  # noqa: E402
from bench_common import PEAK_BYTES_PER_S, timed  # noqa: E402
from deep3d_aerial_amd.dsm import DsmGrid  # noqa: E402

PASSES_MOVED = 20   # per opening: 4 running-extreme passes x (input twice, suffix written and read, output written)


def make_dsm(n, unit, seed=0, empty=0.02):
    """[n,n] fp32 on the GPU: a rolling terrain, 200 box buildings 3 to 30 m wide and 3 to 20 m high, noise on a 1/64 grid, a
    share `empty` of NaN cells."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.arange(n, device="cuda", dtype=torch.float32) + 0.5) * unit
    z = 100.0 + 0.02 * x[None, :] + 0.01 * x[:, None] + 3.0 * torch.sin(x[None, :] / 70.0) * torch.cos(x[:, None] / 90.0)
    rng = np.random.default_rng(seed)
    for _ in range(200):
        w, h = (int(v / unit) for v in rng.uniform(3.0, 30.0, 2))
        i, j = int(rng.integers(0, max(1, n - h))), int(rng.integers(0, max(1, n - w)))
        z[i:i + h, j:j + w] = z[i, j] + float(rng.uniform(3.0, 20.0))
    z = torch.round(z * 64.0) / 64.0 + torch.randint(-2, 3, (n, n), device="cuda", generator=gen).float() / 64.0
    z[torch.rand((n, n), device="cuda", generator=gen) < empty] = float("nan")
    return z.contiguous()


def stats(ms, nbytes=None):
    """bench_common.stats with the measured time as a multiple of the time at 8 TB/s, not the share of it (objects_bench and
    outlines_bench report the same)."""
    med = float(np.median(ms))
    r = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if nbytes is not None:
        floor = nbytes / PEAK_BYTES_PER_S * 1e3
        r.update(bytes=int(nbytes), ms_at_8TBps=round(floor, 4), multiple_of_8TBps=round(med / floor, 2) if floor > 0 else None)
    return r


def pool_open(x, r):
    """The opening of a NaN-free [H,W] raster by max_pool2d on +-inf-padded tensors: a row and a column pass per half."""
    F = torch.nn.functional
    k = 2 * r + 1

    def dil(t):
        t = F.max_pool2d(F.pad(t, (r, r, 0, 0), value=float("-inf")), (1, k), stride=1)
        return F.max_pool2d(F.pad(t, (0, 0, r, r), value=float("-inf")), (k, 1), stride=1)

    t = x[None, None]
    return dil(-dil(-t))[0, 0]


def run(n, unit, radii, runs):
    lib = _lib.load()
    P, st = _geom.ptr, _geom.stream()
    z = make_dsm(n, unit)
    out = torch.empty_like(z)
    scratch, nbytes = _geom.scratch(lib.d3d_dtm_scratch_bytes, n, n, device="cuda")
    cells = n * n
    res = {"size": [n, n], "unit": unit, "runs": runs, "empty_share": round(float(torch.isnan(z).float().mean()), 4), "open": {}}
    full = torch.where(torch.isnan(z), torch.full_like(z, 100.0), z)    # the yardstick has no empty cell
    for r in radii:
        def call(src=z):
            _lib.check(lib.d3d_dtm_open(P(src), P(out), n, n, r, r, P(scratch), nbytes, st), "d3d_dtm_open")

        e = stats(timed(call, runs), 8 * cells)
        e["bytes_moved"] = 4 * cells * PASSES_MOVED
        e["moved_TB_per_s"] = round(e["bytes_moved"] / (e["ms_median"] * 1e-3) / 1e12, 3)
        try:
            state = {}
            e["torch_max_pool2d"] = stats(timed(lambda: state.update(o=pool_open(full, r)), runs if r <= 16 else min(runs, 2)))
            call(full)
            e["torch_max_pool2d"]["same_values"] = bool(torch.equal(state["o"], out))
            e["torch_max_pool2d"]["torch_over_hip"] = round(e["torch_max_pool2d"]["ms_median"] / e["ms_median"], 2)
            state.clear()
        except RuntimeError as err:   # out of memory at the largest windows is a result, not a failure of the tool
            e["torch_max_pool2d"] = {"error": str(err).split("\n")[0][:200]}
        torch.cuda.empty_cache()
        res["open"][str(r)] = e
        print(json.dumps({r: e}), file=sys.stderr, flush=True)
    grid = DsmGrid([0.0, n * unit, 0.0, n * unit], [unit, unit], size=(n, n))
    table = dtm.levels(grid)
    res["levels"] = []
    for rx, ry, dh in table:   # the opening of every level of the default filter, on the same raster
        ms = timed(lambda: _lib.check(lib.d3d_dtm_open(P(z), P(out), n, n, rx, ry, P(scratch), nbytes, st), "d3d_dtm_open"), runs)
        res["levels"].append(dict(stats(ms, 8 * cells), rx=rx, ry=ry, dh=dh))
    del out, scratch, full
    torch.cuda.empty_cache()
    state = {}
    res["dsm_to_dtm"] = stats(timed(lambda: state.update(o=dtm.dsm_to_dtm(z, grid)), max(2, runs // 2)))
    level = state["o"][1]
    res["dsm_to_dtm"]["ground_share"] = round(float((level == 0).float().mean()), 4)
    res["dsm_to_dtm"]["struck_share"] = round(float(((level > 0) & (level < 255)).float().mean()), 4)
    res["bound"] = "unconfirmed (no kernel trace or counters in this run)"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--unit", type=float, default=0.1)
    ap.add_argument("--radii", default="1,16,128,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtm_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/dtm_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S}
    res.update(run(a.size, a.unit, [int(r) for r in a.radii.split(",")], a.runs))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
