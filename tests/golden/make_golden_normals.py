#!/usr/bin/env python3
"""Golden vectors for DESIGN.md §1 row N5 (surface normals from depth), made by RUNNING THE REFERENCE's
ComputeNormals.compute_normal_by_depth (mvs/mvs_cas/models/compute_normals.py:32-82) on CPU torch:

    python tests/golden/make_golden_normals.py

Nothing of the reference is copied: the module is imported in place from /root/reference (sys.dont_write_bytecode keeps
the tree clean).  The .npz files hold data only: seeded depth maps, K, the fp32 inv(K) torch.inverse gives (what the
reference multiplies with, :23), the reference's outputs for nei 1 and 2, and the reference's own error against a float64
evaluation of the same formula with the same inv(K) -- the chord |n_ref - n_f64| (mean and max over the pixels whose summed
vector has a norm >= 1e-3).  tests/test_normals*.py bound the kernel's error by twice those numbers.

Sizes avoid B * (H - 2 nei) * (W - 2 nei) == 3, where the reference's torch.cross (no `dim`) crosses the wrong axis.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("D3D_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REF, "mvs", "mvs_cas", "models"))
import compute_normals as RCN  # noqa: E402

NORM_FLOOR = 1e-3


def intrinsics(h, w, f_scale=1.4, skew=0.0, dc=(0.0, 0.0)):
    f = f_scale * w
    return np.array([[f, skew, (w - 1) / 2.0 + dc[0]], [0, f * 1.01, (h - 1) / 2.0 + dc[1]], [0, 0, 1]], np.float32)


def plane_depth(h, w, K, n_cam, dist):
    """Depth of the plane n . P = dist seen through K (float64, then rounded to float32 by the caller)."""
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.linalg.inv(K.astype(np.float64)) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    n = np.asarray(n_cam, np.float64) / np.linalg.norm(n_cam)
    return (dist / (n @ rays)).reshape(h, w)


def normals_f64(depth, kinv, nei):
    """compute_normals.py:32-82 in float64 with the same fp32 inv(K): returns (normal [B,H,W,3], |summed vector| [B,H,W])."""
    depth = np.asarray(depth, np.float64)
    B, H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    u = np.stack([xs * depth, ys * depth, depth], -1)                     # [B,H,W,3]
    P = np.einsum("bij,bhwj->bhwi", np.asarray(kinv, np.float64).reshape(B, 3, 3), u)
    s = lambda r0, r1, c0, c1: P[:, r0:H - 2 * nei + r0, c0:W - 2 * nei + c0]
    ctr = s(nei, 0, nei, 0)
    x0, y0, x1, y1 = s(nei, 0, 0, 0), s(0, 0, nei, 0), s(nei, 0, 2 * nei, 0), s(2 * nei, 0, nei, 0)
    x0y0, x0y1, x1y0, x1y1 = s(0, 0, 0, 0), s(2 * nei, 0, 0, 0), s(0, 0, 2 * nei, 0), s(2 * nei, 0, 2 * nei, 0)

    def nz(v):
        return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)

    acc = (nz(np.cross(ctr - x1, y1 - ctr)) + nz(np.cross(ctr - x0, y0 - ctr)) + nz(np.cross(ctr - x0y1, x0y0 - ctr))
           + nz(np.cross(x1y0 - ctr, ctr - x1y1)))
    out = np.zeros((B, H, W, 3))
    norm = np.zeros((B, H, W))
    out[:, nei:H - nei, nei:W - nei] = nz(acc)
    norm[:, nei:H - nei, nei:W - nei] = np.linalg.norm(acc, axis=-1)
    return out, norm


def record(name, depth, K):
    depth = np.ascontiguousarray(depth, np.float32)
    K = np.ascontiguousarray(K, np.float32)
    kinv = torch.inverse(torch.from_numpy(K)).numpy()
    out = {"depth": depth, "K": K, "kinv": kinv}
    mod = RCN.ComputeNormals()
    for nei in (1, 2):
        B, H, W = depth.shape
        if H < 2 * nei or W < 2 * nei:
            continue
        assert B * (H - 2 * nei) * (W - 2 * nei) != 3
        ref = mod.compute_normal_by_depth(torch.from_numpy(depth), torch.from_numpy(K), nei).numpy()
        f64, norm = normals_f64(depth, kinv, nei)
        chord = np.linalg.norm(ref - f64, axis=-1)[norm >= NORM_FLOOR]
        out["ref_nei%d" % nei] = ref.astype(np.float32)
        out["ref_chord_mean_nei%d" % nei] = np.float64(chord.mean() if chord.size else 0.0)
        out["ref_chord_max_nei%d" % nei] = np.float64(chord.max() if chord.size else 0.0)
        print("%s nei %d: reference vs float64 chord mean %.3g max %.3g over %d px" % (name, nei, out["ref_chord_mean_nei%d" % nei],
                                                                                       out["ref_chord_max_nei%d" % nei], chord.size))
    np.savez(os.path.join(HERE, "normals_%s.npz" % name), **out)


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(20261015)
    # B = 2, two cameras (the second with skew and an offset principal point), tilted planes at depth ~600, 0.2 % noise
    h, w = 64, 97
    Ks = [intrinsics(h, w), intrinsics(h, w, 1.1, skew=0.7, dc=(3.5, -2.0))]
    d = [plane_depth(h, w, Ks[0], [0.08, -0.05, -1.0], -600.0), plane_depth(h, w, Ks[1], [-0.2, 0.1, -1.0], -640.0)]
    d = np.stack(d) * (1.0 + 0.002 * rng.standard_normal((2, h, w)))
    record("batch2", d, np.stack(Ks))
    # odd size, zero-depth holes (scattered, and a patch whose stencils are all zero) and a step edge: a roof against ground
    h, w = 37, 53
    K = intrinsics(h, w)
    g = plane_depth(h, w, K, [0.05, 0.03, -1.0], -600.0) * (1.0 + 0.002 * rng.standard_normal((h, w)))
    g[8:20, 12:30] -= 25.0                                        # the roof, 25 units closer
    g[rng.uniform(size=(h, w)) < 0.03] = 0.0
    g[24:31, 36:45] = 0.0
    record("holes_edge", g[None], K[None])
    # larger single map, noise-free plane
    h, w = 64, 97
    K = intrinsics(h, w, 1.3)
    record("plane", plane_depth(h, w, K, [0.1, 0.2, -1.0], -580.0)[None], K[None])
    # degenerate: H == 2 nei for nei = 2 (all zeros); nei = 1 still has two interior rows
    h, w = 4, 11
    K = intrinsics(h, w)
    record("thin", (plane_depth(h, w, K, [0.0, 0.1, -1.0], -600.0) * (1.0 + 0.002 * rng.standard_normal((h, w))))[None], K[None])


if __name__ == "__main__":
    main()
