"""CPU checks of the comparison of two point clouds (deep3d_aerial_amd/cloud_compare.py, csrc/cloud_compare.hip).
`nearest_numpy` restates the rule of cloud_compare.py's docstring by brute force over all pairs -- op-by-op fp64, np.rint, argmin
over the candidates in input-index order for the tie rule -- and `nearest_cells` restates it with a cell list for larger clouds;
the two are checked against each other and against hand-computed answers here, and tests/test_cloud_compare_gpu.py compares the
kernel against them bit for bit.  Also: the statistics, the PLY reader, the error clouds, the command line's refusals, the C ABI and
its argument checks, and the operator's refusals."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import test_cloud as TC
from deep3d_aerial_amd import _lib, cloud, cloud_compare as CC

NEW_SYMBOLS = ("d3d_cloud_compare_scratch_bytes", "d3d_cloud_compare_nearest")
CAP, BINS = 1024, 1026


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def _rows(xq, rows, xt, cand, h, e, idx):
    """The nearest of the queries xq[rows] among the targets xt[cand]; cand holds input indices in increasing order, so the first
    minimum of argmin is the lowest input index among equally distant targets.  Writes e[rows] and idx[rows]."""
    if len(cand) == 0 or len(rows) == 0:
        return
    cap2 = h * h
    d = xq[rows][:, None, :] - xt[cand][None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    inside = d2 < cap2
    a = np.argmin(np.where(inside, d2, np.inf), 1)
    found = inside.any(1)
    best = d2[np.arange(len(rows)), a]
    ee = np.minimum(CAP, np.rint(np.sqrt(np.where(found, best, 0.0)) / h * 1024.0).astype(np.int64))
    e[rows] = np.where(found, ee, CAP)
    idx[rows] = np.where(found, cand[a], -1)


def _finish(okq, e, idx):
    e = np.where(okq, e, -1).astype(np.int32)
    idx = np.where(okq, idx, -1).astype(np.int32)
    hist = np.bincount(np.where(idx >= 0, e, BINS - 1)[okq], minlength=BINS).astype(np.int64)
    return e, idx, hist


def nearest_numpy(query, target, grid):
    """(e [nq] int32, idx [nq] int32, hist [1026] int64) of the rule, by brute force over all pairs of keyed points."""
    q, t = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    okq, okt = TC.cells_numpy(q, grid)[0], TC.cells_numpy(t, grid)[0]
    xq, xt, h = q.astype(np.float64), t.astype(np.float64), np.float64(grid.voxel)
    e, idx = np.full(len(q), CAP, np.int64), np.full(len(q), -1, np.int64)
    rows, cand = np.nonzero(okq)[0], np.nonzero(okt)[0]
    step = max(1, (1 << 22) // max(len(cand), 1))
    for s in range(0, len(rows), step):
        _rows(xq, rows[s:s + step], xt, cand, h, e, idx)
    return _finish(okq, e, idx)


def _key(cell):
    return (cell[:, 2] << 42) | (cell[:, 1] << 21) | cell[:, 0]


def nearest_cells(query, target, grid):
    """nearest_numpy with a cell list: the candidates of a query are the keyed targets of the 3 x 3 x 3 cells around its own, in
    increasing input index."""
    q, t = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    okq, cq, _ = TC.cells_numpy(q, grid)
    okt, ct, _ = TC.cells_numpy(t, grid)
    xq, xt, h = q.astype(np.float64), t.astype(np.float64), np.float64(grid.voxel)
    e, idx = np.full(len(q), CAP, np.int64), np.full(len(q), -1, np.int64)
    ti = np.nonzero(okt)[0]
    tk = _key(ct[ti])
    by = np.argsort(tk, kind="stable")
    ti, tk = ti[by], tk[by]
    ukeys, first, count = np.unique(tk, return_index=True, return_counts=True)
    where = {int(u): (int(f), int(c)) for u, f, c in zip(ukeys, first, count)}
    qi = np.nonzero(okq)[0]
    qk = _key(cq[qi])
    by = np.argsort(qk, kind="stable")
    qi, qk = qi[by], qk[by]
    qkeys, qfirst, qcount = np.unique(qk, return_index=True, return_counts=True)
    for u, f, c in zip(qkeys.tolist(), qfirst.tolist(), qcount.tolist()):
        ix, iy, iz = u & ((1 << 21) - 1), (u >> 21) & ((1 << 21) - 1), u >> 42
        near = [where.get(((iz + dz) << 42) | ((iy + dy) << 21) | (ix + dx)) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if min(ix + dx, iy + dy, iz + dz) >= 0 and ix + dx < grid.n[0] and iy + dy < grid.n[1] and iz + dz < grid.n[2]]
        near = [ti[a:a + b] for a, b in filter(None, near)]
        if not near:
            continue
        cand = np.sort(np.concatenate(near))
        for s in range(f, f + c, 512):
            _rows(xq, qi[s:min(s + 512, f + c)], xt, cand, h, e, idx)
    return _finish(okq, e, idx)


def stats_numpy(hist_a, hist_b, h, taus, points):
    """The statistics of the docstring, restated on Python integers and fractions."""
    from fractions import Fraction

    def direction(hist, n):
        hist = [int(v) for v in hist]
        m = sum(hist)
        d = [min(e, CAP) for e in range(BINS)]
        cum = list(itertools.accumulate(hist))
        out = {"points": n, "keyed": m, "beyond": hist[1025],
               "mean": float(Fraction(sum(a * v for a, v in zip(d, hist)), CAP * m)) * h if m else 0.0,
               "rms": math.sqrt(float(Fraction(sum(a * a * v for a, v in zip(d, hist)), CAP * CAP * m))) * h if m else 0.0}
        for p in (50, 90, 95):
            e = min(k for k in range(BINS) if cum[k] >= (p * m + 99) // 100) if m else 0
            out["p%d" % p] = d[e] / 1024 * h
        return out, cum, m

    a, ca, ma = direction(hist_a, points[0])
    b, cb, mb = direction(hist_b, points[1])
    rows = []
    for tau in taus:
        t = math.floor(tau / h * 1024 + 0.5)
        den = ca[t] * mb + cb[t] * ma
        rows.append({"threshold": float(tau), "bin": t, "accuracy": float(Fraction(ca[t], ma)) if ma else 0.0,
                     "completeness": float(Fraction(cb[t], mb)) if mb else 0.0, "fscore": float(Fraction(2 * ca[t] * cb[t], den)) if den else 0.0})
    return {"max_dist": float(h), "cloud": a, "reference": b, "thresholds": rows}


def error_bytes_numpy(xyz, e):
    """The bytes of an error cloud, restated point by point."""
    import struct

    head = ("ply\nformat binary_little_endian 1.0\ncomment error cloud (deep3d_aerial_amd.cloud_compare)\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property int e\nend_header\n" % len(e)).encode("ascii")
    body = b""
    for p, v in zip(np.asarray(xyz, np.float32), [int(v) for v in e]):
        rgb = (128, 128, 128) if v < 0 else (min(255, v >> 1), min(255, (1024 - v) >> 1), 0)
        body += struct.pack("<3f3Bi", float(p[0]), float(p[1]), float(p[2]), rgb[0], rgb[1], rgb[2], v)
    return head + body


# ----------------------------------------------------------------------------------------
# hand-computed cases (shared with tests/test_cloud_compare_gpu.py)
# ----------------------------------------------------------------------------------------
NAN, INF = np.nan, np.inf
NEAR = np.float32(1.5 - 2.0 ** -20)   # 2^-20 short of one cap from 0.5: within the cap, and e rounds up to 1024


def hand_cases():
    """(name, query, target, grid, e, idx, {bin: count}) worked out by hand on the unit grid (h = 1)."""
    g = TC.unit_grid()
    q0 = np.float32([[0.5, 0.5, 0.5]])
    none = np.zeros((0, 3), np.float32)
    face = np.float32([[0.75, 0.5, 0.5], [1.25, 0.5, 0.5]])   # a quarter on either side of the query at the face x = 1
    gone = np.float32([[NAN, 1, 1], [1, INF, 1], [4, 1, 1], [1, -0.5, 1], [9, 9, 9]])
    return [
        ("a query on a target", q0, q0.copy(), g, [0], [0], {0: 1}),
        ("a quarter cap away", q0, np.float32([[0.75, 0.5, 0.5]]), g, [256], [0], {256: 1}),
        ("exactly one cap away: none found", q0, np.float32([[1.5, 0.5, 0.5]]), g, [1024], [-1], {1025: 1}),
        ("2^-20 inside the cap: e rounds up to 1024, and found", q0, np.float32([[NEAR, 0.5, 0.5]]), g, [1024], [0], {1024: 1}),
        ("equal distances across a cell face", np.float32([[1.0, 0.5, 0.5]]), face, g, [256], [0], {256: 1}),
        ("equal distances across a cell face, the targets swapped", np.float32([[1.0, 0.5, 0.5]]), face[::-1].copy(), g, [256], [0], {256: 1}),
        ("duplicate targets: the lowest index", q0, np.float32([[0.9, 0.5, 0.5], [0.75, 0.5, 0.5], [0.75, 0.5, 0.5], [0.75, 0.5, 0.5]]), g,
         [256], [1], {256: 1}),
        ("duplicate queries", np.float32([[0.5, 0.5, 0.5]] * 3), np.float32([[0.5, 1.0, 0.5]]), g, [512] * 3, [0] * 3, {512: 3}),
        ("unkeyed queries enter no count", np.concatenate([gone, q0, gone]), np.float32([[0.75, 0.5, 0.5]]), g, [-1] * 5 + [256] + [-1] * 5,
         [-1] * 5 + [0] + [-1] * 5, {256: 1}),
        # the target at x = -0.1 is 0.2 from the query but outside the grid; the one at 0.6 is 0.5 away
        ("unkeyed targets are nobody's neighbours", np.float32([[0.1, 0.5, 0.5]]),
         np.concatenate([np.float32([[-0.1, 0.5, 0.5]]), gone, np.float32([[0.6, 0.5, 0.5]])]), g, [512], [6], {512: 1}),
        ("only unkeyed targets", q0, gone, g, [1024], [-1], {1025: 1}),
        ("only unkeyed queries", gone, q0, g, [-1] * 5, [-1] * 5, {}),
        ("an empty query", none, q0, g, [], [], {}),
        ("an empty target", np.float32([[0.5, 0.5, 0.5], [NAN, 0, 0], [3.5, 3.5, 3.5]]), none, g, [1024, -1, 1024], [-1, -1, -1], {1025: 2}),
        ("both empty", none, none, g, [], [], {}),
        # (0.875,)*3 and (1.125,)*3: sqrt(3) / 4 apart, e = rint(443.4) = 443, across a cell, a row and a layer
        ("a neighbour across a cell, a row and a layer border", np.float32([[0.875] * 3]), np.float32([[3.5, 3.5, 3.5], [1.125] * 3]), g,
         [443], [1], {443: 1}),
        # the last cell of a row and the first of the next are no neighbours; the grid's corner cells
        ("the end of a row and the grid's corners", np.float32([[3.9, 0.5, 0.5], [0, 0, 0], [3.75, 3.75, 3.75]]),
         np.float32([[0.1, 1.5, 0.5], [0.25, 0, 0], [3.75, 3.5, 3.75]]), g, [1024, 256, 256], [-1, 1, 2], {1025: 1, 256: 2}),
    ]


def hist_of(bins):
    h = np.zeros(BINS, np.int64)
    for k, v in bins.items():
        h[k] = v
    return h


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_the_rule_by_hand(case):
    _, q, t, g, e, idx, bins = case
    for got in (nearest_numpy(q, t, g), nearest_cells(q, t, g)):
        assert got[0].tolist() == e and got[1].tolist() == idx and np.array_equal(got[2], hist_of(bins))
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[2].shape == (BINS,)
        assert got[2].sum() == sum(v >= 0 for v in e)


def random_clouds(seed, nq, nt):
    """Two clouds over (and a little beyond) a 12 x 10 x 6 grid of 0.5 with shared clusters, exact duplicates within and across the
    clouds, and unkeyed points."""
    rng = np.random.default_rng(seed)
    g = cloud.CloudGrid([10.0, 16.0, -3.0, 2.0, 0.0, 2.6], 0.5)
    lo, hi = np.array(g.border[0::2]), np.array(g.border[1::2])
    c = rng.uniform(lo, hi, (3, 3))
    out = []
    for n in (nq, nt):
        xyz = rng.uniform(lo - 0.2, hi + 0.2, (n, 3))
        xyz[: n // 3] = c[rng.integers(0, 3, n // 3)] + rng.normal(0, 0.1, (n // 3, 3))
        xyz = xyz.astype(np.float32)
        if n:
            xyz[rng.integers(0, n, n // 20)] = xyz[rng.integers(0, n, n // 20)]
            bad = rng.integers(0, n, max(n // 50, 1))
            xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.float32([NAN, INF, -INF, 3e38]), len(bad))
        out.append(xyz[rng.permutation(n)])
    if nq and nt:
        k = min(nq, nt) // 10
        out[0][:k] = out[1][:k]   # queries that lie on a target
    return out[0], out[1], g


@pytest.mark.parametrize("seed, nq, nt", [(0, 1, 1), (1, 2, 50), (2, 50, 2), (3, 700, 900), (4, 3000, 2500), (5, 300, 0), (6, 0, 300)])
def test_the_cell_list_is_the_brute_force(seed, nq, nt):
    q, t, g = random_clouds(seed, nq, nt)
    a, b = nearest_numpy(q, t, g), nearest_cells(q, t, g)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    e, idx, hist = a
    assert hist.sum() == (e >= 0).sum() and hist[BINS - 1] == ((e >= 0) & (idx < 0)).sum()
    if min(nq, nt) >= 700:
        assert 0 < (e < 0).sum() < nq // 4 and hist[0] > 0 and hist[BINS - 1] > 0 and 0 < (hist[1:CAP] > 0).sum()
        # the order of the queries does not matter; idx follows a permutation of the targets
        p = np.random.default_rng(nq).permutation(nq)
        ep, ip, hp = nearest_cells(q[p], t, g)
        assert np.array_equal(ep, e[p]) and np.array_equal(ip, idx[p]) and np.array_equal(hp, hist)
        p = np.random.default_rng(nt).permutation(nt)
        ep, ip, hp = nearest_cells(q, t[p], g)
        assert np.array_equal(ep, e) and np.array_equal(hp, hist) and np.array_equal(ip >= 0, idx >= 0)
        assert np.array_equal(t[p][ip[ip >= 0]], t[idx[idx >= 0]], equal_nan=True)   # the same place, whichever duplicate


# ----------------------------------------------------------------------------------------
# the statistics
# ----------------------------------------------------------------------------------------
HIST_A = {0: 2, 256: 1, 512: 1, 1025: 1}
HIST_B = {128: 1, 256: 1, 1024: 2}


def test_the_statistics_by_hand():
    # h = 2, tau = 0.5: t = floor(0.5 / 2 * 1024 + 0.5) = 256.  A: m = 5, cum[256] = 3; B: m = 4, cum[256] = 2.
    # P = 3/5, R = 2/4, F = 2 * 3 * 2 / (3 * 4 + 2 * 5) = 12/22.
    # A: S1 = 256 + 512 + 1024 = 1792, mean = 1792 / 5120 * 2 = 0.7; S2 = 65536 + 262144 + 1048576 = 1376256,
    #    rms = sqrt(1376256 / 5242880) * 2 = sqrt(0.2625) * 2; p50: need 3 -> e = 256 -> 0.5; p90, p95: need 5 -> bin 1025 -> the cap 2.
    # B: S1 = 128 + 256 + 2048 = 2432, mean = 2432 / 4096 * 2 = 1.1875; S2 = 16384 + 65536 + 2097152 = 2179072,
    #    rms = sqrt(2179072 / 4194304) * 2; p50: need 2 -> e = 256 -> 0.5; p90, p95: need 4 -> e = 1024 -> 2.
    r = CC.stats(hist_of(HIST_A), hist_of(HIST_B), 2.0, [0.5, 1.0], points=(7, 4))
    assert r["max_dist"] == 2.0 and sorted(r) == ["cloud", "max_dist", "reference", "thresholds"]
    assert r["cloud"] == {"points": 7, "keyed": 5, "beyond": 1, "mean": 0.7, "rms": math.sqrt(0.2625) * 2.0, "p50": 0.5, "p90": 2.0, "p95": 2.0}
    assert r["reference"] == {"points": 4, "keyed": 4, "beyond": 0, "mean": 1.1875, "rms": math.sqrt(2179072 / 4194304) * 2.0, "p50": 0.5,
                              "p90": 2.0, "p95": 2.0}
    assert r["thresholds"][0] == {"threshold": 0.5, "bin": 256, "accuracy": 0.6, "completeness": 0.5, "fscore": 12 / 22}
    # tau = 1: t = 512: cum_A = 4, cum_B = 2: P = 0.8, R = 0.5, F = 2 * 4 * 2 / (4 * 4 + 2 * 5) = 16/26
    assert r["thresholds"][1] == {"threshold": 1.0, "bin": 512, "accuracy": 0.8, "completeness": 0.5, "fscore": 16 / 26}
    assert r == stats_numpy(hist_of(HIST_A), hist_of(HIST_B), 2.0, [0.5, 1.0], (7, 4))
    # lists, arrays and tensors; a single threshold; no point counts
    r1 = CC.stats(hist_of(HIST_A).tolist(), torch.from_numpy(hist_of(HIST_B)), 2, 0.5)
    assert r1["thresholds"] == r["thresholds"][:1] and r1["cloud"]["points"] is None and r1["cloud"]["mean"] == 0.7
    # a query that found nothing counts the cap, and never falls under a threshold: the largest bin is 1023
    r2 = CC.stats(hist_of({1025: 3}), hist_of({1024: 3}), 2.0, [1.999])
    assert r2["thresholds"][0]["bin"] == 1023 and r2["thresholds"][0]["accuracy"] == 0.0 and r2["thresholds"][0]["fscore"] == 0.0
    assert r2["cloud"]["mean"] == 2.0 and r2["reference"]["mean"] == 2.0 and r2["cloud"]["beyond"] == 3 and r2["reference"]["beyond"] == 0
    # the largest counts stay exact integers
    big = (1 << 31) - 1
    r3 = CC.stats(hist_of({1: big}), hist_of({1: big}), 1.0, [0.5])
    assert r3["thresholds"][0]["fscore"] == 1.0 and r3["cloud"]["mean"] == 1 / 1024 and r3["cloud"]["rms"] == 1 / 1024


def test_thresholds_at_zero_and_at_the_cap_are_refused_and_no_keyed_point_gives_zeros():
    a, b = hist_of(HIST_A), hist_of(HIST_B)
    assert CC.threshold_bin(0.5, 2.0) == 256 and CC.threshold_bin(1.999, 2.0) == 1023 and CC.threshold_bin(0.001, 2.0) == 1
    for tau in (0.0005, 0.0, -1.0, 2.0, 1.9995, 5.0):   # bins 0, 0, < 0, 1024, 1024, > 1024
        with pytest.raises(ValueError, match="1 .. 1023"):
            CC.stats(a, b, 2.0, [0.5, tau])
    for tau in (NAN, INF, "1", True):
        with pytest.raises(ValueError, match="threshold"):
            CC.stats(a, b, 2.0, [tau])
    with pytest.raises(ValueError, match="at least one"):
        CC.stats(a, b, 2.0, [])
    for h in (0.0, -1.0, NAN, INF, "2", True):
        with pytest.raises(ValueError, match="max_dist"):
            CC.stats(a, b, h, [0.5])
    for bad in (a[:-1], np.concatenate([a, a]), -a):
        with pytest.raises(ValueError, match="1026"):
            CC.stats(bad, b, 2.0, [0.5])
    zero = {"points": 0, "keyed": 0, "beyond": 0, "mean": 0.0, "rms": 0.0, "p50": 0.0, "p90": 0.0, "p95": 0.0}
    r = CC.stats(hist_of({}), hist_of({}), 2.0, [0.5], points=(0, 0))
    assert r["cloud"] == zero and r["reference"] == zero
    assert r["thresholds"] == [{"threshold": 0.5, "bin": 256, "accuracy": 0.0, "completeness": 0.0, "fscore": 0.0}]
    r = CC.stats(a, hist_of({}), 2.0, [0.5], points=(7, 3))   # one side without a keyed point
    assert r["thresholds"][0] == {"threshold": 0.5, "bin": 256, "accuracy": 0.6, "completeness": 0.0, "fscore": 0.0}
    assert r["reference"] == dict(zero, points=3) and r == stats_numpy(a, hist_of({}), 2.0, [0.5], (7, 3))


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def ply_bytes(fmt, elements):
    """A PLY file: elements = [(name, count, [(type, property) | "list ..." text], body bytes)]."""
    head = ["ply", "format %s 1.0" % fmt, "comment a test file"]
    body = b""
    for name, count, props, data in elements:
        head.append("element %s %d" % (name, count))
        head += ["property %s" % (p if isinstance(p, str) else "%s %s" % p) for p in props]
        body += data
    return ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + body


def test_read_xyz_ply(tmp_path):
    rng = np.random.default_rng(7)
    m = 11
    xyz = rng.normal(size=(m, 3)).astype(np.float32)
    write = lambda name, data: (tmp_path / name).write_bytes(data) and str(tmp_path / name)
    # float coordinates, properties of every width before, between and after them, a face element after the vertices
    dt = np.dtype([("id", "<u2"), ("x", "<f4"), ("flag", "i1"), ("y", "<f4"), ("z", "<f4"), ("t", "<f8"), ("red", "u1"), ("n", "<u4"), ("s", "<i2")])
    rec = np.zeros(m, dt)
    for k, a in enumerate("xyz"):
        rec[a] = xyz[:, k]
    rec["id"], rec["t"], rec["red"] = np.arange(m), rng.normal(size=m), 200
    props = [("ushort", "id"), ("float", "x"), ("char", "flag"), ("float32", "y"), ("float", "z"), ("double", "t"), ("uchar", "red"), ("uint", "n"),
             ("int16", "s")]
    faces = b"".join(bytes([3]) + np.int32([0, 1, 2]).tobytes() for _ in range(4))
    path = write("mesh.ply", ply_bytes("binary_little_endian", [("vertex", m, props, rec.tobytes()),
                                                                ("face", 4, ["list uchar int vertex_indices"], faces)]))
    got = CC.read_xyz_ply(path)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(TC.bits(got), TC.bits(xyz))
    # double coordinates are rounded to fp32; z before x
    xyz64 = rng.normal(size=(m, 3)) * 1e3
    dt = np.dtype([("z", "<f8"), ("x", "<f8"), ("y", "<f8"), ("intensity", "<u2")])
    rec = np.zeros(m, dt)
    for k, a in enumerate("xyz"):
        rec[a] = xyz64[:, k]
    path = write("lidar.ply", ply_bytes("binary_little_endian", [("vertex", m, [("double", "z"), ("float64", "x"), ("double", "y"),
                                                                                 ("uint16", "intensity")], rec.tobytes())]))
    assert np.array_equal(TC.bits(CC.read_xyz_ply(path)), TC.bits(xyz64.astype(np.float32)))
    # a file write_cloud_ply wrote, and an empty one
    src = cloud.write_cloud_ply(str(tmp_path / "c.ply"), xyz, xyz, np.zeros((m, 3), np.uint8), np.ones(m, np.int32))
    assert np.array_equal(TC.bits(CC.read_xyz_ply(src)), TC.bits(xyz))
    src = cloud.write_cloud_ply(str(tmp_path / "e.ply"), xyz[:0], None, None, np.ones(0, np.int32))
    assert CC.read_xyz_ply(src).shape == (0, 3)
    # an error cloud reads back too
    (tmp_path / "err.ply").write_bytes(CC.error_cloud_bytes(xyz, np.arange(m, dtype=np.int32) - 1))
    assert np.array_equal(TC.bits(CC.read_xyz_ply(str(tmp_path / "err.ply"))), TC.bits(xyz))
    # refusals
    v3 = [("float", "x"), ("float", "y"), ("float", "z")]
    body = xyz.tobytes()
    for name, data, msg in (
            ("ascii.ply", ply_bytes("ascii", [("vertex", m, v3, b"0 0 0\n" * m)]), "ASCII"),
            ("big.ply", ply_bytes("binary_big_endian", [("vertex", m, v3, xyz.astype(">f4").tobytes())]), "big-endian"),
            ("noz.ply", ply_bytes("binary_little_endian", [("vertex", m, v3[:2] + [("float", "w")], body)]), "no property z"),
            ("intx.ply", ply_bytes("binary_little_endian", [("vertex", m, [("int", "x")] + v3[1:], body)]), "float or double"),
            ("list.ply", ply_bytes("binary_little_endian", [("vertex", m, v3 + ["list uchar int k"], body)]), "scalar"),
            ("face_first.ply", ply_bytes("binary_little_endian", [("face", 0, ["list uchar int vertex_indices"], b""), ("vertex", m, v3, body)]),
             "first element"),
            ("short.ply", ply_bytes("binary_little_endian", [("vertex", m, v3, body[:-1])]), "bytes"),
            ("twice.ply", ply_bytes("binary_little_endian", [("vertex", m, v3 + [("float", "x")], body)]), "twice"),
            ("not.ply", b"plyish\n" + body, "not a PLY")):
        with pytest.raises(ValueError, match=msg):
            CC.read_xyz_ply(write(name, data))
    # cloud.read_cloud_ply stays as it is: it still refuses a mesh
    with pytest.raises(ValueError):
        cloud.read_cloud_ply(str(tmp_path / "mesh.ply"))


def test_the_error_cloud_bytes_by_hand():
    import struct

    xyz = np.float32([[1, 2, 3], [4, 5, 6], [7, 8, 9], [0.5, 0.25, 0.125], [NAN, 0, 0]])
    e = np.int32([0, 1024, 511, 3, -1])
    data = CC.error_cloud_bytes(xyz, e)
    assert data == error_bytes_numpy(xyz, e) == CC.error_cloud_bytes(torch.from_numpy(xyz), torch.from_numpy(e))
    head, body = data[:data.index(b"end_header\n") + 11], data[data.index(b"end_header\n") + 11:]
    assert head.decode().split("\n")[3:11] == ["element vertex 5", "property float x", "property float y", "property float z", "property uchar red",
                                               "property uchar green", "property uchar blue", "property int e"]
    assert len(body) == 5 * 19
    rows = [struct.unpack_from("<3f3Bi", body, 19 * k) for k in range(5)]
    assert rows[0] == (1.0, 2.0, 3.0, 0, 255, 0, 0)       # on the reference: green (512 clamps to 255)
    assert rows[1] == (4.0, 5.0, 6.0, 255, 0, 0, 1024)    # at or past the cap: red (512 clamps to 255)
    assert rows[2] == (7.0, 8.0, 9.0, 255, 255, 0, 511)   # 511 >> 1 = 255, 513 >> 1 = 256 -> 255
    assert rows[3] == (0.5, 0.25, 0.125, 1, 255, 0, 3)    # 3 >> 1 = 1, 1021 >> 1 = 510 -> 255
    assert rows[4][3:] == (128, 128, 128, -1) and math.isnan(rows[4][0])
    assert CC.error_cloud_bytes(xyz[:0], e[:0]).endswith(b"end_header\n")
    for bad_xyz, bad_e in ((xyz.astype(np.float64), e), (xyz, e.astype(np.int64)), (xyz, e[:4]), (xyz, np.int32([0, 1, 2, 3, 1025])),
                           (xyz, np.int32([0, 1, 2, 3, -2]))):
        with pytest.raises(ValueError):
            CC.error_cloud_bytes(bad_xyz, bad_e)


def test_the_command_line_refuses_before_it_writes(capsys, tmp_path):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    out = tmp_path / "out"
    full = ["--cloud", a, "--reference", b, "--border=0,8,0,4,-1,1", "--max_dist=0.5", "--threshold=0.1,0.25", "--json", str(out / "r.json"),
            "--out_accuracy", str(out / "ea.ply"), "--out_completeness", str(out / "eb.ply")]
    drop = lambda k: full[:k] + full[k + 2:] if not full[k].count("=") else full[:k] + full[k + 1:]
    for argv in (drop(0), drop(2), drop(4), drop(5), drop(6),
                 full[:4] + ["--border=0,8,0,4"] + full[5:], full[:5] + ["--max_dist=0"] + full[6:], full[:5] + ["--max_dist=1e-9", "--threshold=3e-10"] + full[7:],
                 full[:6] + ["--threshold=0.1,0.5"] + full[7:], full[:6] + ["--threshold=0.0001"] + full[7:],
                 full[:6] + ["--threshold=0.1,x"] + full[7:], full[:6] + ["--threshold=-1"] + full[7:],
                 full[:7] + ["--json", str(out / "r.txt")] + full[9:], full[:9] + ["--out_accuracy", str(out / "ea.xyz")] + full[11:],
                 full[:11] + ["--out_completeness", str(out / "ea.ply")], full[:9] + ["--out_accuracy", a] + full[11:]):
        with pytest.raises(SystemExit):
            CC.main(argv)
    err = capsys.readouterr().err
    for text in ("--cloud is required", "--reference is required", "--border is required", "--max_dist is required", "--threshold is required",
                 "max_dist must be finite", "2^21", "1 .. 1023", "T[,T...]", "--json must end in .json", "--out_accuracy must end in .ply",
                 "the same file", "overwrite an input"):
        assert text in err, text
    assert not out.exists()


# ----------------------------------------------------------------------------------------
# the library and the operator
# ----------------------------------------------------------------------------------------
def test_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    assert sorted(_lib.STRUCTS) == ["d3d_mesh_grid_t", "d3d_mesh_view_t", "d3d_ortho_view_t"]   # no new struct
    assert len(_lib.SIGNATURES["d3d_cloud_compare_nearest"]) == 18
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_build_flags() == b""
    scratch = lib.d3d_cloud_compare_scratch_bytes
    assert scratch.restype is ctypes.c_size_t
    assert scratch(0, 0) > 0 and scratch(1_000_000, 0) > 0 and scratch(0, 1_000_000) >= 16 * 1_000_000
    assert scratch(1_000_000, 1_000_000) >= 16 * 1_000_000
    big = (1 << 31) - 1
    assert scratch(big, big) >= 16 * big and scratch(0, big) >= 16 * big and scratch(big, 0) > 0
    for bad in (-1, 1 << 31):
        assert scratch(bad, 10) == 0 and scratch(10, bad) == 0 and scratch(bad, bad) == 0, bad


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    nq, nt = 10, 7
    need = lib.d3d_cloud_compare_scratch_bytes(nq, nt)
    order = ["qx", "qk", "qo", "nq", "tx", "tk", "to", "nt", "nx", "ny", "nz", "h", "s", "sb", "e", "idx", "hist", "st"]
    ok = dict(qx=P(1), qk=P(2), qo=P(3), nq=nq, tx=P(4), tk=P(5), to=P(6), nt=nt, nx=16, ny=8, nz=4, h=0.5, s=P(7), sb=need, e=P(8), idx=P(9),
              hist=P(10), st=None)
    size = dict(qx=12 * nq, qk=8 * nq, qo=8 * nq, tx=12 * nt, tk=8 * nt, to=8 * nt, s=need, e=4 * nq, idx=4 * nq, hist=8 * BINS)
    # every pair of buffers: the second begins on the last byte of the first, and the first on the last byte of the second
    alias = []
    for a, b in itertools.combinations(size, 2):
        alias.append((dict([(b, ctypes.c_void_p(ok[a].value + size[a] - 1))]), b"alias"))
        alias.append((dict([(a, ctypes.c_void_p(ok[b].value + size[b] - 1))]), b"alias"))
    assert len(alias) == 90
    TC._expect(lib, lib.d3d_cloud_compare_nearest, ok, order,
               [(dict([(name, None)]), b"null") for name in size] +
               [(dict(nq=-1), b"n_query"), (dict(nq=1 << 31), b"n_query"), (dict(nt=-1), b"n_target"), (dict(nt=1 << 31), b"n_target"),
                (dict(nx=0), b"grid"), (dict(ny=1 << 21), b"grid"), (dict(nz=-3), b"grid"),
                (dict(h=0.0), b"cap"), (dict(h=-1.0), b"cap"), (dict(h=math.nan), b"cap"), (dict(h=math.inf), b"cap"),
                (dict(sb=need - 1), b"scratch"), (dict(sb=0), b"scratch"),
                # no query, no target: the scratch and the histogram are still needed
                (dict(nq=0, qx=None, qk=None, qo=None, e=None, idx=None, s=None), b"null"),
                (dict(nt=0, tx=None, tk=None, to=None, hist=None), b"null"),
                (dict(nq=0, nt=0, sb=0), b"scratch")] + alias)


def test_the_operator_refuses_cpu_tensors_bad_dtypes_and_shapes():
    g = TC.unit_grid()
    xyz = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.prepare(xyz, g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.nearest(xyz, xyz.clone(), g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CC.compare(xyz, xyz.clone(), g.border, 1.0, [0.5])
    for bad in (xyz.double(), torch.zeros(5, 2), torch.zeros(15), torch.zeros(5, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="query"):
            CC.nearest(bad, xyz, g)
        with pytest.raises(ValueError, match="target"):
            CC.nearest(xyz, bad, g)
        with pytest.raises(ValueError, match="xyz"):
            CC.prepare(bad, g)
    with pytest.raises(TypeError, match="CloudGrid"):
        CC.nearest(xyz, xyz, [0, 4, 0, 4, 0, 4])
    with pytest.raises(TypeError, match="CloudGrid"):
        CC.prepare(xyz, None)
    with pytest.raises(TypeError, match="Tensor"):
        CC.nearest(np.zeros((5, 3), np.float32), xyz, g)
    with pytest.raises(TypeError, match="Tensor"):
        CC.nearest(xyz, None, g)
    for kw, msg in ((dict(max_dist=0.0), "max_dist"), (dict(max_dist=1e-9, thresholds=[5e-10]), "2\\^21"), (dict(border=[0, 4, 0, 4]), "six"),
                    (dict(thresholds=[1.0]), "1 .. 1023"), (dict(thresholds=[]), "at least one")):
        with pytest.raises(ValueError, match=msg):
            CC.compare(**dict(dict(cloud_xyz=xyz, reference_xyz=xyz, border=g.border, max_dist=1.0, thresholds=[0.5]), **kw))


def test_the_kernels_use_integer_atomic_add_only_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    for name, n_atomics in (("cloud_compare.hip", 2), ("cloud_search.h", 0)):
        hip = strip(open(_lib.CSRC + "/" + name).read())
        assert set(re.findall(r"\batomic\w*", hip)) == ({"atomicAdd"} if n_atomics else set())
        assert not re.search(r"unsafeAtomic|atomicAdd\s*\(\s*\(?\s*(float|double)\s*\*|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
        # every atomicAdd is a statement: its result is not used
        assert len(re.findall(r"(?:^|[;{}\)])\s*atomicAdd\(", hip, re.M)) == len(re.findall(r"\batomicAdd\(", hip)) == n_atomics
        assert "fma" not in hip
    hip = strip(open(_lib.CSRC + "/cloud_compare.hip").read())
    # one on the unsigned LDS histogram, one on the unsigned 64-bit histogram in memory
    assert "__shared__ unsigned bins[CC_BINS]" in hip and "atomicAdd(&bins[" in hip and "atomicAdd(hist + b, (unsigned long long)v)" in hip
    assert re.search(r"unsigned long long\* __restrict__ hist\)", hip) and '#include "cloud_search.h"' in hip
    # the search helpers have one statement, in cloud_search.h: the outliers and the merge include them, and no .hip file restates
    # the lower bound, the overlap check, the tile's LDS arrays, the occupancy query or the private names of the shared constants
    search = strip(open(_lib.CSRC + "/cloud_search.h").read())
    assert search.count("keys[mid] < k") == 1 and "int bound[CLOUD_BOUNDS][SEARCH_BLOCK]" in search and "int edge[2][CLOUD_BOUNDS]" in search
    assert search.count("hipOccupancyMaxActiveBlocksPerMultiprocessor") == 1 and "(cloud.hip)" not in search
    sources = {name: strip(open(_lib.CSRC + "/" + name).read()) for name in sorted(os.listdir(_lib.CSRC)) if name.endswith((".hip", ".h"))}
    for name, text in sources.items():
        if name.endswith(".hip"):
            for gone in ("keys[mid] < k", "struct CloudRange", "cloud_apart", "struct SearchRange", "bool search_apart"):
                assert gone not in text, (name, gone)
            assert not re.search(r"\bom_apart\b", text), name   # (as a word: geom_shared.h's geom_apart is the one pair test)
            assert not re.search(r"\bbound\[|\bedge\[\w+\]\[|hipOccupancyMaxActiveBlocksPerMultiprocessor", text), name
    for name in ("cloud.hip", "cloud_outliers.hip", "cloud_compare.hip"):
        assert '#include "cloud_search.h"' in sources[name]
        assert not re.search(r"\bC[OL]_(AXIS_MAX|DROPPED|CAP|BOUNDS|AHEAD)\b|\bCO_(BLOCK|WAVES)\b|\bCC_(AHEAD|BLOCK|WAVES)\b", sources[name]), name
    for name in ("cloud_outliers.hip", "cloud_compare.hip"):
        assert all(call in sources[name] for call in ("search_tile(", "search_walk(", "search_gather(")), name
    assert "cloud_lower(" in sources["cloud.hip"] and "search_apart(" in sources["cloud.hip"] and "search_apart(" in sources["ortho_mesh.hip"]
    # one count check under csrc/, one gather kernel in the library
    assert sum(len(re.findall(r"count_ok\(long long", text)) for text in sources.values()) == 1
    assert sum(len(re.findall(r"__global__[^;{]*\bcloud\w*_gather_kernel\(", text)) for text in sources.values()) == 1
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bcloud_compare\.hip\b", make, re.M) and re.search(r"^HDRS :=.*\bcloud_search\.h\b", make, re.M)
    assert "-ffp-contract=off" in make


def test_the_package_states_the_clouds_checks_and_keys_once():
    pkg = os.path.dirname(cloud.__file__)
    text = {name: open(os.path.join(pkg, name)).read() for name in sorted(os.listdir(pkg)) if name.endswith(".py")}
    # no module reaches into cloud_compare for an underscore name, by import or by attribute
    for name, src in text.items():
        assert not re.search(r"from \.cloud_compare import[^\n]*\b_\w+|\bcloud_compare\._\w+", src), name
    # d3d_cloud_keys is called from one place, and the sort of its keys stands in cloud.py alone among the stages on the grid
    assert [name for name, src in text.items() for _ in re.findall(r"d3d_cloud_keys\(", src)] == ["cloud.py"]
    for name in ("cloud_outliers.py", "cloud_compare.py", "cloud_register.py", "mesh_compare.py"):
        assert "torch.sort(" not in text[name], name
    assert "cloud.sorted_keys(" in text["cloud_outliers.py"] and "cloud.sorted_keys(" in text["cloud_compare.py"]
    # the spelled-out number checks, the hand-typed PLY headers and the private writers are gone from the package
    for name, src in text.items():
        assert not re.search(r"isinstance\(\w+, bool\) or not isinstance", src) or name == "_geom.py", name
        if name in ("cloud.py", "cloud_outliers.py", "cloud_compare.py", "cloud_register.py"):
            assert "format binary_little_endian 1.0\"," not in src and "def _write(" not in src and "host = lambda" not in src, name
    assert text["_geom.py"].count("isinstance(x, bool) or not isinstance") == 2
    # the four vertex-only writers go through the one in _geom
    for name, n in (("cloud.py", 1), ("cloud_compare.py", 1), ("cloud_register.py", 1), ("mesh_compare.py", 1)):
        assert text[name].count("_geom.record_ply_bytes(") == n, name
