"""The comparison of a surface mesh with a reference cloud (csrc/mesh_sample.hip, deep3d_aerial_amd/mesh_compare.py) on synthetic
meshes: a jittered grid of --faces triangles on a smooth surface, sampled at its mean edge length (mostly n_f = 1 .. 2) and at a
quarter of it.  Per mesh and spacing: device-event ms (one warm-up, then --runs timed calls, each on its own events: median, min,
max) of d3d_mesh_sample_count (the count kernel and the scan together), d3d_mesh_sample_emit and d3d_mesh_sample_face_error, the
bytes each must move (computed from the shapes) as a time at 8 TB/s and the share of the measured time that is; the whole
mesh_compare.compare against a reference cloud of as many points as the mesh has faces (its host reads included), with its split
into the sampling, the two key-and-sort passes and the two searches, while the samples stay under --compare_max_samples; and, while
they stay under --torch_max_samples, the sampling as plain torch in the same run: repeat_interleave of the faces by n_f^2 and the
rule's arithmetic on gathered corners, with the share of samples whose bits agree.  One very uneven mesh: ten faces of n_f = 2000
among 10^6 faces of n_f = 1, its emit time per sample beside the even mesh's.  The face error on "all samples in 64 faces" (the most
contended case); with --variant_library SO (a `make MESH_SAMPLE=plain` build: one set of atomics per sample) both builds run on the
same tensors, taking turns, and must give the same bits.  What bounds the kernels is not measured here: no kernel trace and no
counters are taken.  Prints one JSON line (and writes --out).

    python tools/mesh_compare_bench.py [--runs 5] [--faces 1e6,1e7,5e7] [--variant_library SO] [--out profiles/mesh_compare_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_common import PEAK_BYTES_PER_S, bind, stats, timed  # noqa: E402
from deep3d_aerial_amd import _geom, _lib, cloud, cloud_compare, mesh_compare  # noqa: E402

CELL = 0.1


def make_mesh(m, seed=0):
    """(vertices, faces, border): a side x side grid of cells of CELL, two triangles a cell (2 side^2 = about m faces), the inner
    nodes moved by up to a quarter of a cell, on z = a smooth surface; the faces in row order."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    side = max(1, int(math.isqrt(m // 2)))
    k = torch.arange((side + 1) * (side + 1), device="cuda")
    i, j = k % (side + 1), k // (side + 1)
    inner = ((i > 0) & (i < side) & (j > 0) & (j < side)).double()
    u = (torch.rand(((side + 1) * (side + 1), 2), device="cuda", generator=gen).double() - 0.5) * 0.5 * inner[:, None]
    x, y = (i + u[:, 0]) * CELL, (j + u[:, 1]) * CELL
    z = 2.0 + torch.sin(x * 0.7) * torch.cos(y * 0.5)
    v = torch.stack([x, y, z], 1).float().contiguous()
    c = torch.arange(side * side, device="cuda")
    a = (c // side) * (side + 1) + c % side
    f = torch.stack([torch.stack([a, a + 1, a + side + 2], 1), torch.stack([a, a + side + 2, a + side + 1], 1)], 1).reshape(-1, 3).int().contiguous()
    L = CELL * side
    return v, f, [-1.0, L + 1.0, -1.0, L + 1.0, 0.0, 4.0]


def mean_edge(v, f):
    d = v.double()
    A, B, C = d[f[:, 0].long()], d[f[:, 1].long()], d[f[:, 2].long()]
    return float(((A - B).norm(dim=1) + (B - C).norm(dim=1) + (C - A).norm(dim=1)).mean() / 3.0)


class Sampler(object):
    """The three entries on one mesh and spacing, on buffers allocated once."""

    def __init__(self, v, f, s):
        self.lib, self.v, self.f, self.s = _lib.load(), v, f, float(s)
        self.n, self.m = int(v.shape[0]), int(f.shape[0])
        self.counts = torch.empty((self.m,), dtype=torch.int32, device="cuda")
        self.offsets = torch.empty((self.m + 1,), dtype=torch.int32, device="cuda")
        self.totals = torch.empty((2,), dtype=torch.int64, device="cuda")
        self.scratch, self.nbytes = _geom.scratch(self.lib.d3d_mesh_sample_scratch_bytes, self.m, device="cuda")
        self.count()
        self.S, self.clipped = self.totals.tolist()
        if self.clipped or self.S >= 1 << 31:
            raise ValueError("%d samples, %d clipped faces" % (self.S, self.clipped))
        self.xyz = torch.empty((self.S, 3), dtype=torch.float32, device="cuda")
        self.face = torch.empty((self.S,), dtype=torch.int32, device="cuda")

    def count(self):
        P = _geom.ptr
        _lib.check(self.lib.d3d_mesh_sample_count(P(self.v), self.n, P(self.f), self.m, self.s, P(self.scratch), self.nbytes, P(self.counts),
                                                  P(self.offsets), P(self.totals), _geom.stream()), "d3d_mesh_sample_count")

    def emit(self):
        P = _geom.ptr
        _lib.check(self.lib.d3d_mesh_sample_emit(P(self.v), self.n, P(self.f), self.m, P(self.offsets), self.S, P(self.xyz), P(self.face),
                                                 _geom.stream()), "d3d_mesh_sample_emit")


def face_error_call(lib, e, face, m, out):
    P = _geom.ptr
    _lib.check(lib.d3d_mesh_sample_face_error(P(e), P(face), int(e.shape[0]), m, P(out[0]), P(out[1]), P(out[2]), _geom.stream()),
               "d3d_mesh_sample_face_error")


def face_error_buffers(m):
    return (torch.empty((m,), dtype=torch.int64, device="cuda"), torch.empty((m,), dtype=torch.int32, device="cuda"),
            torch.empty((m,), dtype=torch.int32, device="cuda"))


def torch_sample(v, f, counts, offsets, S):
    """The rule as plain torch: repeat_interleave of the faces by n_f^2 and the same arithmetic on gathered corners."""
    nn = counts.long()
    face = torch.repeat_interleave(torch.arange(f.shape[0], device="cuda"), nn, output_size=S)
    t = torch.arange(S, device="cuda") - offsets.long()[face]
    n = torch.sqrt(nn.double()).round().long()[face]
    r = torch.sqrt(t.double()).long()
    r = torch.where(r * r > t, r - 1, r)
    r = torch.where((r + 1) * (r + 1) <= t, r + 1, r)
    c = t - r * r
    k, odd = c >> 1, c & 1
    p, q, w = (3 * (n - r) - 2 + odd).double(), (3 * k + 1 + odd).double(), (3 * (r - k) + 1 - 2 * odd).double()
    d = v.double()
    fl = f.long()[face]
    x = ((p[:, None] * d[fl[:, 0]] + q[:, None] * d[fl[:, 1]]) + w[:, None] * d[fl[:, 2]]) / (3 * n).double()[:, None]
    return x.float(), face.int()


def run(m, which, runs, a):
    v, f, border = make_mesh(m)
    n, m = int(v.shape[0]), int(f.shape[0])
    edge = mean_edge(v, f)
    s = edge if which == "mean_edge" else 0.25 * edge
    sm = Sampler(v, f, s)
    S = sm.S
    res = {"faces": m, "vertices": n, "spacing": which, "spacing_value": s, "samples": S, "samples_per_face": round(S / m, 3), "runs": runs}
    # count: the faces and the vertices in, the counts out; scan: the counts in twice, the offsets out
    res["count_and_scan"] = stats(timed(sm.count, runs), 12 * m + 12 * n + 4 * m + 3 * 4 * m)
    # emit: 16 bytes a sample out; the faces, vertices and offsets the samples name in once
    res["emit"] = stats(timed(sm.emit, runs), 16 * S + 12 * m + 12 * n + 4 * m)
    res["emit"]["ns_per_sample"] = round(res["emit"]["ms_median"] * 1e6 / max(S, 1), 5)
    gen = torch.Generator(device="cuda").manual_seed(1)
    e = torch.randint(-1, 1025, (S,), device="cuda", generator=gen, dtype=torch.int32)
    out = face_error_buffers(m)
    # face error: e and face in, the three outputs cleared and then touched once a face (the atomics return nothing)
    res["face_error"] = stats(timed(lambda: face_error_call(sm.lib, e, sm.face, m, out), runs), 8 * S + 2 * 16 * m)
    del e, out
    if S <= a.torch_max_samples:
        state = {}
        t_ms = timed(lambda: state.update(r=torch_sample(v, f, sm.counts, sm.offsets, S)), runs)
        h_ms = timed(lambda: (sm.count(), sm.emit()), runs)
        tx, tf = state["r"]
        same = (tx.view(torch.int32) == sm.xyz.view(torch.int32)).all(1)
        res["torch_sampling"] = {"torch": stats(t_ms), "hip_count_scan_emit": stats(h_ms),
                                 "torch_over_hip": round(float(np.median(t_ms)) / float(np.median(h_ms)), 3),
                                 "same_face": bool(torch.equal(tf, sm.face)), "share_of_samples_with_equal_bits": round(float(same.double().mean()), 9)}
        state.clear()
        del tx, tf, same
    else:
        res["torch_sampling"] = "not run: %d samples are more than --torch_max_samples %d (its temporaries)" % (S, a.torch_max_samples)
    torch.cuda.empty_cache()
    if S <= a.compare_max_samples:
        gen = torch.Generator(device="cuda").manual_seed(2)
        L = border[1] - 1.0
        u = torch.rand((m, 3), device="cuda", generator=gen)
        x, y = u[:, 0] * L, u[:, 1] * L
        ref = torch.stack([x, y, 2.0 + torch.sin(x * 0.7) * torch.cos(y * 0.5) + (u[:, 2] - 0.5) * 0.02], 1).float().contiguous()
        del u, x, y
        cap, taus = 3 * CELL, [0.5 * CELL, CELL]
        g = cloud.CloudGrid(border, cap)
        state = {}
        res["compare"] = stats(timed(lambda: state.update(r=mesh_compare.compare(v, f, ref, border, cap, taus, s)), runs))
        res["compare"]["result"] = state["r"][0]
        state.clear()
        res["compare_split"] = {
            "sample": stats(timed(lambda: state.update(r=mesh_compare.sample(v, f, s)), runs)),
            "prepare_samples": stats(timed(lambda: state.update(pa=cloud_compare.prepare(sm.xyz, g)), runs)),
            "prepare_reference": stats(timed(lambda: state.update(pb=cloud_compare.prepare(ref, g)), runs))}
        res["compare_split"]["nearest_samples_to_reference"] = stats(timed(lambda: state.update(n1=cloud_compare.nearest(sm.xyz, ref, g, state["pa"], state["pb"])), runs))
        res["compare_split"]["nearest_reference_to_samples"] = stats(timed(lambda: state.update(n2=cloud_compare.nearest(ref, sm.xyz, g, state["pb"], state["pa"])), runs))
        state.clear()
        del ref
    else:
        res["compare"] = "not run: %d samples are more than --compare_max_samples %d" % (S, a.compare_max_samples)
    res["bound"] = "not measured (no kernel trace or counters in this run)"
    return res


def uneven(runs, even_ns):
    """Ten faces of n_f = 2000 among 10^6 faces of n_f = 1."""
    v, f, _ = make_mesh(1_000_000)
    s = 4.0 * CELL   # every grid face is shorter: n_f = 1
    L = 1999.5 * s
    big_v = torch.tensor([[[0.0, -10.0 - 2 * L * k, 0.0], [L, -10.0 - 2 * L * k, 0.0], [0.3 * L, -10.0 - 2 * L * k - 0.6 * L, 1.0]] for k in range(10)],
                         device="cuda").reshape(-1, 3)
    base = int(v.shape[0])
    big_f = (torch.arange(30, device="cuda").reshape(10, 3) + base).int()
    m = int(f.shape[0])
    at = torch.linspace(0, m - 1, 10, device="cuda").long()
    f = torch.cat([f, big_f])
    order = torch.arange(m + 10, device="cuda")
    order[at], order[m:] = torch.arange(m, m + 10, device="cuda"), at   # the large faces spread over the face list
    sm = Sampler(torch.cat([v, big_v]).contiguous(), f[order].contiguous(), s)
    r = {"faces": m + 10, "large_faces": 10, "n_f_of_the_large_faces": int(math.isqrt(int(sm.counts.max()))), "samples": sm.S,
         "count_and_scan": stats(timed(sm.count, runs)), "emit": stats(timed(sm.emit, runs))}
    r["emit"]["ns_per_sample"] = round(r["emit"]["ms_median"] * 1e6 / sm.S, 5)
    r["even_mesh_emit_ns_per_sample"] = even_ns
    return r


def contended(runs, variant):
    """All samples in 64 faces: 2^24 samples, 2^18 consecutive ones a face."""
    S, m = 1 << 24, 64
    gen = torch.Generator(device="cuda").manual_seed(3)
    e = torch.randint(-1, 1025, (S,), device="cuda", generator=gen, dtype=torch.int32)
    face = (torch.arange(S, device="cuda") >> 18).int()
    lib = _lib.load()
    out = face_error_buffers(m)
    r = {"samples": S, "faces": m}
    if not variant:
        r["production_run_reduced"] = stats(timed(lambda: face_error_call(lib, e, face, m, out), runs), 8 * S)
        r["variant"] = "not run: no --variant_library"
        return r
    other, out2 = bind(variant), face_error_buffers(m)
    a_ms, b_ms = [], []
    for _ in range(runs):   # taking turns
        a_ms += timed(lambda: face_error_call(lib, e, face, m, out), 1)
        b_ms += timed(lambda: face_error_call(other, e, face, m, out2), 1)
    r.update(production_run_reduced=stats(a_ms, 8 * S), variant_one_atomic_set_per_sample=stats(b_ms, 8 * S), variant_library=variant,
             same_bits=bool(all(torch.equal(x, y) for x, y in zip(out, out2))),
             variant_over_production=round(float(np.median(b_ms)) / float(np.median(a_ms)), 3))
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--faces", default="1e6,1e7,5e7")
    ap.add_argument("--torch_max_samples", type=int, default=100_000_000, help="the torch formulation runs while the samples stay under this")
    ap.add_argument("--compare_max_samples", type=int, default=400_000_000, help="the whole compare runs while the samples stay under this")
    ap.add_argument("--variant_library", default=None, metavar="SO",
                    help="a MESH_SAMPLE=plain build of the library whose face error is timed beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_compare_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/mesh_compare_bench.py measures the GPU kernels: no GPU here")
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "runs": []}
    even_ns = None
    for m in [int(float(x)) for x in a.faces.split(",")]:
        for which in ("mean_edge", "quarter_of_mean_edge"):
            try:
                res["runs"].append(run(m, which, a.runs, a))
            except (ValueError, torch.cuda.OutOfMemoryError) as err:   # 2^31 samples or more, or no room for them
                res["runs"].append({"faces": m, "spacing": which, "not_run": str(err).split("\n")[0]})
                torch.cuda.empty_cache()
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
            if even_ns is None and "emit" in res["runs"][-1]:
                even_ns = res["runs"][-1]["emit"]["ns_per_sample"]
    res["uneven"] = uneven(a.runs, even_ns)
    print(json.dumps(res["uneven"]), file=sys.stderr, flush=True)
    res["face_error_all_samples_in_64_faces"] = contended(a.runs, a.variant_library)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
