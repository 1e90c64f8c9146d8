"""The comparison of two point clouds on the GPU (csrc/cloud_compare.hip, cloud_compare.prepare / nearest / compare): e, idx and
hist bit-equal to the numpy restatements of tests/test_cloud_compare.py -- on the hand-computed cases, on empty and unkeyed clouds,
on a cell of 5000 targets queried from every cell around it, on single-query cells past one scan block, on query cells that straddle
waves and tiles, on query cells without a target in reach, on a lattice of exact ties, on more tiles than the launched grid holds,
on a surface with floaters against a shifted sample of it in any point order --; the statistics of compare(); and the file tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_cloud as TC
import test_cloud_compare as TCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRID_CAP = 2048   # CC_GRID_CAP of csrc/cloud_compare.hip: the workgroups launched at most (fewer where fewer are resident), a tile of 256 queries each


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 3)).cuda()


def _check(query, target, grid, want=None):
    """The GPU's e, idx and hist against the restatement (want, or brute force for small clouds and the cell list for others)."""
    from deep3d_aerial_amd import cloud_compare as CC

    q, t = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    if want is None:
        want = TCC.nearest_numpy(q, t, grid) if len(q) * max(len(t), 1) <= 1 << 25 else TCC.nearest_cells(q, t, grid)
    e, idx, hist = CC.nearest(_cuda(q), _cuda(t), grid)
    assert e.is_cuda and e.dtype == torch.int32 and idx.dtype == torch.int32 and hist.dtype == torch.int64
    assert tuple(e.shape) == (len(q),) and tuple(idx.shape) == (len(q),) and tuple(hist.shape) == (TCC.BINS,)
    assert np.array_equal(hist.cpu().numpy(), want[2])
    assert np.array_equal(e.cpu().numpy(), want[0])
    assert np.array_equal(idx.cpu().numpy(), want[1])
    return want


def _in_voxels(vox, seed, h=1.0):
    """One point in each listed cell (a list of (ix, iy, iz), repeats allowed) of a grid from the origin, at a random place in it."""
    rng = np.random.default_rng(seed)
    return ((np.asarray(vox, np.float64).reshape(-1, 3) + rng.uniform(0.01, 0.99, (len(vox), 3))) * h).astype(np.float32)


# ----------------------------------------------------------------------------------------
# sizes and runs
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TCC.hand_cases(), ids=lambda c: c[0])
def test_the_hand_cases(case):
    _, q, t, g, e, idx, bins = case
    w = _check(q, t, g)
    assert w[0].tolist() == e and w[1].tolist() == idx and np.array_equal(w[2], TCC.hist_of(bins))


def test_no_query_no_target_and_only_unkeyed_points_on_either_side():
    g = TC.unit_grid()
    some = _in_voxels([(k % 4, k // 4 % 4, k // 16) for k in range(64)] * 5, 1)
    none = np.zeros((0, 3), np.float32)
    gone = np.float32([[np.nan, 1, 1], [4, 1, 1], [1, -0.5, 1], [1, 1, np.inf], [9, 9, 9]] * 60)   # more than one tile of them
    assert _check(none, some, g)[2].sum() == 0
    w = _check(some, none, g)
    assert w[2][TCC.BINS - 1] == len(some) and (w[0] == 1024).all() and (w[1] == -1).all()
    assert _check(none, none, g)[2].sum() == 0
    w = _check(gone, some, g)
    assert w[2].sum() == 0 and (w[0] == -1).all() and (w[1] == -1).all()
    w = _check(some, gone, g)
    assert w[2][TCC.BINS - 1] == len(some) and (w[1] == -1).all()
    # unkeyed points among the others, on both sides
    w = _check(np.concatenate([gone[:7], some, gone[:3]]), np.concatenate([gone[:11], some[::-1] + np.float32(0.001), gone[:2]]), g)
    assert w[2].sum() == len(some) and (w[0][:7] == -1).all() and (w[1][7:-3] >= 11).all()


def test_the_prepared_clouds_serve_both_directions():
    from deep3d_aerial_amd import cloud_compare as CC

    q, t, g = TCC.random_clouds(4, 3000, 2500)
    dq, dt = _cuda(q), _cuda(t)
    pq, pt = CC.prepare(dq, g), CC.prepare(dt, g)
    assert pq[0].dtype == torch.int64 and pq[1].dtype == torch.int64 and np.array_equal(pq[0].cpu().numpy(), np.sort(TC.keys_numpy(q, g)))
    want = TCC.nearest_numpy(q, t, g)
    for got in (CC.nearest(dq, dt, g, pq, pt), CC.nearest(dq, dt, g, None, pt), CC.nearest(dq, dt, g, pq)):
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
    back = TCC.nearest_numpy(t, q, g)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(CC.nearest(dt, dq, g, pt, pq), back))
    with pytest.raises(ValueError, match="query_prepared"):
        CC.nearest(dq, dt, g, pt, pt)
    with pytest.raises(TypeError, match="target_prepared"):
        CC.nearest(dq, dt, g, pq, pt[0])
    with pytest.raises(ValueError, match="target_prepared"):
        CC.nearest(dq, dt, g, pq, (pt[0], pt[1].int()))
    with pytest.raises(RuntimeError, match="alias"):   # a cloud against itself needs a copy
        CC.nearest(dq, dq, g)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one GPU"):
            CC.nearest(dq, dt.to("cuda:1"), g)


def test_5000_targets_in_one_cell_queried_from_it_and_the_26_cells_around_it():
    rng = np.random.default_rng(1)
    g = TC.unit_grid(5, 5, 5)
    t = np.concatenate([_in_voxels([(2, 2, 2)] * 5000 + [(2, 2, 1), (1, 2, 2), (3, 3, 3), (0, 0, 0)], 2), np.float32([[2.5, 2.5, 2.5]] * 3)])
    t = t[rng.permutation(len(t))]
    around = [(x, y, z) for z in (1, 2, 3) for y in (1, 2, 3) for x in (1, 2, 3)]
    q = np.concatenate([_in_voxels(around * 20 + [(2, 2, 2)] * 300 + [(0, 4, 4), (4, 0, 2), (0, 1, 0)] * 5, 3), np.float32([[2.5, 2.5, 2.5]] * 2)])
    q = q[rng.permutation(len(q))]
    w = _check(q, t, g, TCC.nearest_cells(q, t, g))
    assert (w[0] == 0).sum() == 2 and w[2][TCC.BINS - 1] > 0 and (w[1] >= 0).sum() > 600


@pytest.mark.parametrize("n", [4097, 2 * 4096 + 1])
def test_one_query_per_cell_past_one_and_two_scan_tiles(n):
    from deep3d_aerial_amd import cloud

    g = cloud.CloudGrid([0.0, 100.0, 0.0, 100.0, 0.0, 2.0], 1.0)
    k = np.arange(n)
    q = _in_voxels(np.stack([k % 100, k // 100 % 100, k // 10000], 1), n)
    q = q[np.random.default_rng(n).permutation(n)]
    t = np.random.default_rng(n + 1).uniform([0, 0, 0], [100, 100, 2], (6000, 3)).astype(np.float32)
    w = _check(q, t, g, TCC.nearest_cells(q, t, g))
    assert 0 < w[2][TCC.BINS - 1] < n and (w[2][:1024] > 0).sum() > 200


def test_query_cells_that_straddle_waves_and_tiles():
    from deep3d_aerial_amd import cloud

    lengths = [1, 2, 63, 64, 65, 255, 256, 257] * 3
    g = cloud.CloudGrid([0.0, 24.0, 0.0, 1.0, 0.0, 1.0], 1.0)   # the cells in a row: a cell's targets are those of the cells beside it
    vox = np.repeat(np.arange(len(lengths)), lengths)
    q = _in_voxels(np.stack([vox, 0 * vox, 0 * vox], 1), 8)
    tv = np.repeat(np.arange(24), [3, 0, 0, 5, 1, 0, 7, 2] * 3)   # some cells hold no target
    t = _in_voxels(np.stack([tv, 0 * tv, 0 * tv], 1), 9)
    t = t[np.random.default_rng(3).permutation(len(t))]
    want = _check(q, t, g, TCC.nearest_cells(q, t, g))                     # the queries already in key order
    assert 0 < want[2][TCC.BINS - 1] < len(q)
    p = np.random.default_rng(10).permutation(len(q))
    _check(q[p], t, g, (want[0][p], want[1][p], want[2]))                    # shuffled
    for skip in (1, 37):   # a shifted start: the cells meet the wave and tile boundaries elsewhere
        _check(q[skip:], t, g, TCC.nearest_cells(q[skip:], t, g))


def test_query_cells_whose_window_holds_no_target_next_to_ones_that_do():
    from deep3d_aerial_amd import cloud

    rng = np.random.default_rng(5)
    g = cloud.CloudGrid([0.0, 40.0, 0.0, 6.0, 0.0, 6.0], 1.0)
    t = np.concatenate([rng.uniform([0, 0, 0], [9, 6, 6], (400, 3)), rng.uniform([30, 2, 2], [31, 3, 3], (10, 3))]).astype(np.float32)
    q = rng.uniform([0, 0, 0], [40, 6, 6], (5000, 3)).astype(np.float32)
    w = _check(q, t, g, TCC.nearest_cells(q, t, g))
    far = (q[:, 0] > 11) & (q[:, 0] < 28)
    assert (w[1][far] == -1).all() and (w[1][q[:, 0] < 8] >= 0).any() and (w[1][q[:, 0] > 29] >= 0).any() and w[2][TCC.BINS - 1] > 2000
    # targets only beyond the last query cell, and only before the first
    _check(q[q[:, 0] < 20], t[400:], g)
    _check(q[q[:, 0] > 20], t[:400], g)


def test_exact_ties_on_a_lattice_go_to_the_lowest_input_index():
    from deep3d_aerial_amd import cloud

    rng = np.random.default_rng(6)
    g = cloud.CloudGrid([0.0, 6.0, 0.0, 6.0, 0.0, 3.0], 1.0)
    ax = lambda a, b: np.arange(a, b + 1e-9, 0.25)
    t = np.stack(np.meshgrid(ax(0.5, 5.5), ax(0.5, 5.5), ax(0.5, 2.5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    t = t[rng.permutation(len(t))]                       # an order unrelated to the keys
    pick = t[rng.choice(len(t), 1500, replace=False)].astype(np.float64)
    q = np.concatenate([pick[:500] + 0.125,              # a lattice cube's centre: eight targets sqrt(3) / 8 away
                        pick[500:1000] + [0.125, 0, 0],  # an edge's middle: two targets 1/8 away
                        pick[1000:] + [0.125, 0.125, 0]]).astype(np.float32)   # a face's middle: four
    q = q[rng.permutation(len(q))]
    want = TCC.nearest_numpy(q, t, g)
    d = q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    ties = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert (ties >= 2).mean() > 0.8 and (ties == 8).any() and (ties == 4).any()   # (fewer at the lattice's faces)
    assert np.array_equal(want[1], np.argmax(d2 == d2.min(1, keepdims=True), 1))  # the first of the equally near, by input index
    _check(q, t, g, want)
    _check(q, t[::-1].copy(), g)                          # and with the input order reversed


def test_more_tiles_than_one_pass_of_the_grid():
    """The entry launches at most GRID_CAP workgroups and each takes one tile of 256 queries per pass: GRID_CAP * 256 queries fill
    one pass of the largest grid, and 257 more make a further pass of at least one full tile and one tile of a single query."""
    from deep3d_aerial_amd import cloud

    n = GRID_CAP * 256 + 257
    assert n == 524545
    rng = np.random.default_rng(7)
    g = cloud.CloudGrid([0.0, 8.0, 0.0, 8.0, 0.0, 4.0], 1.0)
    t = rng.uniform([0, 0, 0], [8, 8, 4], (50, 3)).astype(np.float32)
    q = rng.uniform([-0.1, 0, 0], [8, 8, 4], (n, 3)).astype(np.float32)
    w = _check(q, t, g, TCC.nearest_numpy(q, t, g))
    assert w[2].sum() < n and w[2][TCC.BINS - 1] > n // 4 and (w[2][:1025] > 0).sum() > 800 and len(set(w[1].tolist())) == 51


# ----------------------------------------------------------------------------------------
# a surface with floaters against a shifted sample of it
# ----------------------------------------------------------------------------------------
def surfaces(seed, n=20000, floaters=200):
    """(cloud, reference, border, cap): n points of a jittered surface over 40 x 40 plus floaters and a few points outside the
    border, against another sample of the same surface moved by (0.05, 0, 0.1) that stops at x = 36."""
    rng = np.random.default_rng(seed)

    def sample(m, dx, dz, x1):
        x, y = rng.uniform(0, x1, m), rng.uniform(-20, 20, m)
        return np.stack([x + dx, y, 3.0 + np.sin(0.5 * x) * np.cos(0.4 * y) + rng.normal(0, 0.03, m) + dz], 1)

    a = np.concatenate([sample(n, 0, 0, 40.0), rng.uniform([0, -20, 0], [40, 20, 6], (floaters, 3)), rng.uniform([-5, -25, -3], [45, 25, 9], (50, 3))])
    b = np.concatenate([sample(n, 0.05, 0.1, 36.0), rng.uniform([-5, -25, -3], [45, 25, 9], (20, 3))])
    return (a[rng.permutation(len(a))].astype(np.float32), b[rng.permutation(len(b))].astype(np.float32), [0.0, 40.0, -20.0, 20.0, 0.0, 6.0], 0.5)


def test_the_surface_both_directions_the_statistics_and_any_point_order():
    from deep3d_aerial_amd import cloud, cloud_compare as CC

    a, b, border, h = surfaces(0)
    g = cloud.CloudGrid(border, h)
    taus = [0.1, 0.2, 0.35]
    ab, ba = TCC.nearest_cells(a, b, g), TCC.nearest_cells(b, a, g)
    want = TCC.stats_numpy(ab[2], ba[2], h, taus, (len(a), len(b)))

    def run(x, y):
        result, found = CC.compare(_cuda(x), _cuda(y), border, h, taus)
        assert sorted(found) == ["cloud", "reference"] and all(t.is_cuda and t.dtype == torch.int32 for pair in found.values() for t in pair)
        return result, [t.cpu().numpy() for t in found["cloud"] + found["reference"]]

    result, (ea, ia, eb, ib) = run(a, b)
    assert result == want == CC.stats(ab[2], ba[2], h, taus, (len(a), len(b)))
    assert np.array_equal(ea, ab[0]) and np.array_equal(ia, ab[1]) and np.array_equal(eb, ba[0]) and np.array_equal(ib, ba[1])
    for row in result["thresholds"]:
        assert 0 < row["accuracy"] < 1 and 0 < row["completeness"] < 1 and 0 < row["fscore"] < 1
    assert result["cloud"]["beyond"] > 100 > result["reference"]["beyond"] and result["cloud"]["keyed"] < result["cloud"]["points"]
    assert 0 < result["cloud"]["p50"] <= result["cloud"]["p90"] <= result["cloud"]["p95"] <= h
    # a permutation of either cloud: the same result; e follows the cloud's order, idx names the same place
    rng = np.random.default_rng(2)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    r2, (ea2, ia2, eb2, ib2) = run(a[pa], b[pb])
    assert r2 == result and np.array_equal(ea2, ea[pa]) and np.array_equal(eb2, eb[pb])
    assert np.array_equal(ia2 >= 0, ia[pa] >= 0) and np.array_equal(ib2 >= 0, ib[pb] >= 0)
    assert np.array_equal(b[pb][ia2[ia2 >= 0]], b[ia[pa][ia[pa] >= 0]]) and np.array_equal(a[pa][ib2[ib2 >= 0]], a[ib[pb][ib[pb] >= 0]])
    ab2 = TCC.nearest_cells(a[pa], b[pb], g)   # and idx is the rule's on the permuted clouds: the lowest new index of a tie
    assert np.array_equal(ia2, ab2[1]) and np.array_equal(ea2, ab2[0])


# ----------------------------------------------------------------------------------------
# the file tool
# ----------------------------------------------------------------------------------------
def test_the_file_tool_writes_the_result_and_both_error_clouds_byte_for_byte(tmp_path):
    from deep3d_aerial_amd import cloud, cloud_compare as CC

    a, b, border, h = surfaces(3, 3000, 40)
    src_a = cloud.write_cloud_ply(str(tmp_path / "a.ply"), a, None, None, np.ones(len(a), np.int32))
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("intensity", "<u2")])   # the reference as a LiDAR export in doubles
    rec = np.zeros(len(b), dt)
    for k, f in enumerate("xyz"):
        rec[f] = b[:, k]
    src_b = tmp_path / "b.ply"
    src_b.write_bytes(TCC.ply_bytes("binary_little_endian", [("vertex", len(b), [("double", "x"), ("double", "y"), ("double", "z"),
                                                                                  ("ushort", "intensity")], rec.tobytes())]))
    out = tmp_path / "cli"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.cloud_compare", "--cloud", src_a, "--reference", str(src_b),
           "--border=%s" % ",".join(repr(v) for v in border), "--max_dist=%r" % h, "--threshold=0.15,0.3", "--json", str(out / "r.json"),
           "--out_accuracy", str(out / "ea.ply"), "--out_completeness", str(out / "eb.ply")]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    result, found = CC.compare(_cuda(a), _cuda(b), border, h, [0.15, 0.3])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and json.loads(lines[0]) == result == json.loads((out / "r.json").read_text())
    assert 0 < result["thresholds"][0]["fscore"] < result["thresholds"][1]["fscore"] < 1
    ea, eb = found["cloud"][0].cpu().numpy(), found["reference"][0].cpu().numpy()
    assert (ea == -1).any() and np.array_equal(ea, TCC.nearest_cells(a, b, cloud.CloudGrid(border, h))[0])
    assert (out / "ea.ply").read_bytes() == TCC.error_bytes_numpy(a, ea)
    assert (out / "eb.ply").read_bytes() == TCC.error_bytes_numpy(b, eb)
