"""d3d_normals_from_depth (csrc/normals.hip) at the map size of the fusion tests, 2752 x 1856, B = 1: device-event time per map
with and without the encoded output, bytes from shapes, achieved TB/s and its share of the measured copy rate (6.3 TB/s) and
of the HBM peak (8.0 TB/s), and the output against the float64 restatement of compute_normals.py:32-82 (tests/test_normals.py)
on a tilted plane at depth ~600 with 0.2 % depth noise.  Prints one JSON line (and writes it to --out).

    python tools/normals_bench.py [--iters 200] [--out profiles/normals_bench.json]

Timing: a device sleep first holds the queue while the host enqueues the timed launches, so they run back to back and the
events measure the kernels, not the host's launch rate."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from deep3d_aerial_amd import _lib, ops  # noqa: E402


def scene(h, w, noise, seed=0):
    rng = np.random.default_rng(seed)
    K = np.array([[1.4 * w, 0, (w - 1) / 2.0], [0, 1.4 * w, (h - 1) / 2.0], [0, 0, 1]], np.float64)
    n = np.array([0.12, -0.07, -1.0])
    n /= np.linalg.norm(n)
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    d = (-600.0 / (n @ rays)).reshape(h, w) * (1.0 + noise * rng.standard_normal((h, w)))
    return d.astype(np.float32), K.astype(np.float32)


def timed_us(launch, iters):
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(2e7))   # ~ several ms of device time: the host enqueues everything below meanwhile
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--h", type=int, default=1856)
    ap.add_argument("--w", type=int, default=2752)
    ap.add_argument("--nei", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench needs the GPU (no CPU timing is reported)")
    import test_normals as TN

    lib = _lib.load()
    h, w, nei = a.h, a.w, a.nei
    d, K = scene(h, w, 0.002)
    depth = torch.from_numpy(d).cuda()
    kinv = ops.normals_kinv(K)
    kp = ctypes.cast(kinv.data_ptr(), ctypes.POINTER(ctypes.c_float))
    normal = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    enc = torch.empty_like(normal)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()

    def run(with_enc):
        return lambda: _lib.check(lib.d3d_normals_from_depth(p(depth), kp, 1, h, w, nei, p(normal), p(enc) if with_enc else None, st),
                                  "d3d_normals_from_depth")

    res = {"tool": "normals_bench", "map": [h, w], "B": 1, "nei": nei, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for tag, with_enc in (("normal", False), ("normal+encoded", True)):
        us = timed_us(run(with_enc), a.iters)
        nbytes = h * w * (4 + 12 + (12 if with_enc else 0))
        tbs = nbytes / us / 1e6
        res[tag] = {"us_per_map": round(us, 2), "bytes": nbytes, "TB_s": round(tbs, 3), "share_of_6.3": round(tbs / 6.3, 3),
                    "share_of_8.0": round(tbs / 8.0, 3)}
    # the copy rate of this card in the same run, for scale: one read + one write of the normal map's bytes
    src = torch.empty((h, w, 3), dtype=torch.float32, device="cuda").fill_(1.0)
    dst = torch.empty_like(src)
    us = timed_us(lambda: dst.copy_(src), a.iters)
    res["copy_same_bytes"] = {"us": round(us, 2), "TB_s": round(2 * src.numel() * 4 / us / 1e6, 3)}
    # accuracy at this size against the float64 restatement (pixels whose summed vector is >= 1e-3: all of a plane)
    run(True)()
    torch.cuda.synchronize()
    got = normal.cpu().numpy()[None]
    f64, norm = TN.normals_f64(d[None], kinv.numpy(), nei)
    mean, mx = TN.chord_stats(got, f64, norm)
    res["chord_vs_float64"] = {"mean": float("%.3g" % mean), "max": float("%.3g" % mx), "noise": 0.002}
    res["encoded_is_(n+1)/2"] = bool(torch.equal(enc, (normal + 1.0) * 0.5))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
