"""CPU checks of the cloud's outlier removal (deep3d_aerial_amd/cloud_outliers.py, csrc/cloud_outliers.hip).
`neighbours_numpy` restates the rule of cloud_outliers.py's docstring by brute force over all pairs -- op-by-op fp64, np.rint,
exact Python integers for the statistics -- and `neighbours_cells` restates it with a cell list for larger clouds; the two are
checked against each other and against hand-computed answers here, and tests/test_cloud_outliers_gpu.py compares the kernels
against them bit for bit.  Also: the settings, both command lines, the pipeline's up-front validation, the C ABI and its argument
checks, and the operator's refusals."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import test_cloud as TC
from deep3d_aerial_amd import _lib, cloud, cloud_outliers as CO, pipeline, predict

NEW_SYMBOLS = ("d3d_cloud_outliers_scratch_bytes", "d3d_cloud_outliers_distances")
CAP, K_MAX = 1024, 32


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def _smallest(x, rows, cand, other, h):
    """(E [len(rows), 32] int64, nn [len(rows)]) of the points x[rows] over the candidates x[cand]; other [rows, cand] is false
    where the candidate is the point itself."""
    cap2 = h * h
    with np.errstate(over="ignore", invalid="ignore"):
        d = x[rows][:, None, :] - x[cand][None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        inside = (d2 < cap2) & other
        q = np.sqrt(np.where(inside, d2, 0.0)) / h * 1024.0
    e = np.where(inside, np.minimum(CAP, np.rint(q).astype(np.int64)), CAP)
    e = np.where(other, e, 1 << 40)                                    # the point itself is no candidate ...
    e = np.sort(np.concatenate([e, np.full((len(rows), K_MAX), CAP, np.int64)], 1), 1)[:, :K_MAX]   # ... a missing one counts 1024
    return np.minimum(e, CAP), inside.sum(1)


def neighbours_numpy(xyz, grid):
    """(ok [n] bool, E [n, 32] int64: the 32 smallest e of every keyed point in increasing order, nn [n] int64), by brute force
    over all pairs of keyed points; rows of unkeyed points are not meaningful."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok = TC.cells_numpy(xyz, grid)[0]
    x, h = xyz.astype(np.float64), np.float64(grid.voxel)
    idx = np.nonzero(ok)[0]
    E, nn = np.full((len(xyz), K_MAX), CAP, np.int64), np.zeros(len(xyz), np.int64)
    for s in range(0, len(idx), 256):
        rows = idx[s:s + 256]
        E[rows], nn[rows] = _smallest(x, rows, idx, rows[:, None] != idx[None, :], h)
    return ok, E, nn


def neighbours_cells(xyz, grid):
    """neighbours_numpy with a cell list: the candidates of a point are the keyed points of the 3 x 3 x 3 cells around its own."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok, cell, _ = TC.cells_numpy(xyz, grid)
    x, h = xyz.astype(np.float64), np.float64(grid.voxel)
    idx = np.nonzero(ok)[0]
    key = (cell[idx, 2] << 42) | (cell[idx, 1] << 21) | cell[idx, 0]
    by = np.argsort(key, kind="stable")
    idx, key = idx[by], key[by]
    ukeys, first, count = np.unique(key, return_index=True, return_counts=True)
    where = {int(u): (int(f), int(c)) for u, f, c in zip(ukeys, first, count)}
    E, nn = np.full((len(xyz), K_MAX), CAP, np.int64), np.zeros(len(xyz), np.int64)
    for u, (f, c) in where.items():
        ix, iy, iz = u & ((1 << 21) - 1), (u >> 21) & ((1 << 21) - 1), u >> 42
        near = [where.get(((iz + dz) << 42) | ((iy + dy) << 21) | (ix + dx)) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if min(ix + dx, iy + dy, iz + dz) >= 0 and ix + dx < grid.n[0] and iy + dy < grid.n[1] and iz + dz < grid.n[2]]
        cand = np.concatenate([idx[a:a + b] for a, b in filter(None, near)])
        for s in range(f, f + c, 512):
            rows = idx[s:min(s + 512, f + c)]
            E[rows], nn[rows] = _smallest(x, rows, cand, rows[:, None] != cand[None, :], h)
    return ok, E, nn


def outliers_from(found, k, alpha, min_neighbours):
    """{"D", "nn", "keep", "sums", "info"} of the rule from (ok, E, nn) of one of the two restatements."""
    ok, E, nn = found
    D = np.where(ok, E[:, :k].sum(1), -1).astype(np.int32)
    nn = np.where(ok, nn, -1).astype(np.int32)
    m = int(ok.sum())
    s1 = sum(int(d) for d in D[ok])
    s2 = sum(int(d) * int(d) for d in D[ok])
    mu = s1 / m if m else 0.0
    sigma = math.sqrt(m * s2 - s1 * s1) / m if m else 0.0
    T = None if alpha is None else math.floor(mu + alpha * sigma)
    keep = ok & (nn >= min_neighbours) & (True if T is None else D <= T)
    return {"D": D, "nn": nn, "keep": keep, "sums": (m, s1, s2),
            "info": {"points": len(D), "keyed": m, "kept": int(keep.sum()), "mu": mu, "sigma": sigma, "threshold": T}}


def outliers_numpy(xyz, grid, k=8, alpha=2.0, min_neighbours=0):
    return outliers_from(neighbours_numpy(xyz, grid), k, alpha, min_neighbours)


# ----------------------------------------------------------------------------------------
# hand-computed cases (shared with tests/test_cloud_outliers_gpu.py)
# ----------------------------------------------------------------------------------------
NAN, INF = np.nan, np.inf
NEAR = np.float32(1.5 - 2.0 ** -20)   # 2^-20 short of one radius from 0.5: within the radius, and e rounds up to 1024


def hand_cases():
    """(name, xyz, grid, k, alpha, min_neighbours, D, nn, keep) with D, nn and keep worked out by hand."""
    g = TC.unit_grid()
    three = np.float32([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 1.0, 0.5]])   # distances 1/4, 1/2 and sqrt(5)/4: e = 256, 512, 572
    five = np.float32([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [2.5, 2.5, 2.5], [3.5, 0.5, 0.5], [3.5, 0.5, 0.5]])
    gone = np.float32([[NAN, 1, 1], [1, INF, 1], [1, 1, -INF], [4, 1, 1], [1, -0.5, 1], [9, 9, 9]])
    return [
        ("two points a quarter radius apart", three[:2], g, 1, None, 1, [256, 256], [1, 1], [1, 1]),
        ("a missing neighbour counts 1024", three[:2], g, 2, None, 1, [1280, 1280], [1, 1], [1, 1]),
        ("three points, k = 2", three, g, 2, None, 2, [768, 828, 1084], [2, 2, 2], [1, 1, 1]),
        ("exactly one radius apart: e = 1024 and no neighbour", np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]), g, 1, None, 1,
         [1024, 1024], [0, 0], [0, 0]),
        ("just inside the radius: e rounds up to 1024, and a neighbour", np.float32([[0.5, 0.5, 0.5], [NEAR, 0.5, 0.5]]), g, 1, None, 1,
         [1024, 1024], [1, 1], [1, 1]),
        ("a duplicate pair", np.float32([[1.25, 2.5, 3.75]] * 2), g, 1, 0.0, 1, [0, 0], [1, 1], [1, 1]),
        ("fewer than k candidates, k = 32", three[:2], g, 32, None, 1, [256 + 31 * 1024] * 2, [1, 1], [1, 1]),
        ("unkeyed points are nobody's neighbours", np.concatenate([gone, three[:2], gone]), g, 1, 2.0, 0,
         [-1] * 6 + [256, 256] + [-1] * 6, [-1] * 6 + [1, 1] + [-1] * 6, [0] * 6 + [1, 1] + [0] * 6),
        ("only unkeyed points", gone, g, 8, 2.0, 0, [-1] * 6, [-1] * 6, [0] * 6),
        ("one point", three[:1], g, 8, 2.0, 0, [8192], [0], [1]),
        ("one point fails the radius test", three[:1], g, 8, 2.0, 1, [8192], [0], [0]),
        # D = 256, 256, 1024, 0, 0: m = 5, S1 = 1536, S2 = 1179648, mu = 307.2, m S2 - S1^2 = 3538944 = 1881.2..^2,
        # sigma = 376.24..: alpha 1 gives T = floor(683.4) = 683, alpha 2 T = floor(1059.7) = 1059, alpha 0 T = 307
        ("the threshold, alpha = 1", five, g, 1, 1.0, 0, [256, 256, 1024, 0, 0], [1, 1, 0, 1, 1], [1, 1, 0, 1, 1]),
        ("the threshold, alpha = 2", five, g, 1, 2.0, 0, [256, 256, 1024, 0, 0], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1]),
        ("the threshold, alpha = 0", five, g, 1, 0.0, 0, [256, 256, 1024, 0, 0], [1, 1, 0, 1, 1], [1, 1, 0, 1, 1]),
        ("alpha and the radius test together", five, g, 1, 2.0, 1, [256, 256, 1024, 0, 0], [1, 1, 0, 1, 1], [1, 1, 0, 1, 1]),
        ("all-equal D: sigma = 0 keeps everything", np.float32([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 2.5]]), g, 3, 0.0, 0,
         [3072] * 3, [0] * 3, [1] * 3),
        # (0.875, 0.875, 0.875) and (1.125, 1.125, 1.125): sqrt(3) / 4 apart, e = rint(443.4) = 443, across a cell, a row and a layer
        ("neighbours across a cell, a row and a layer border", np.float32([[0.875] * 3, [1.125] * 3]), g, 1, None, 1, [443, 443], [1, 1], [1, 1]),
        # at the grid's faces: the cells (0,0,0) and (3,3,3); the last cell of a row and the first of the next are no neighbours
        ("the grid's faces and the end of a row", np.float32([[0, 0, 0], [0.25, 0, 0], [3.75, 3.75, 3.75], [3.75, 3.5, 3.75], [3.9, 0.5, 0.5],
                                                               [0.1, 1.5, 0.5]]), g, 1, None, 1, [256, 256, 256, 256, 1024, 1024],
         [1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0]),
    ]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_the_rule_by_hand(case):
    _, xyz, g, k, alpha, m, D, nn, keep = case
    for found in (neighbours_numpy(xyz, g), neighbours_cells(xyz, g)):
        got = outliers_from(found, k, alpha, m)
        assert got["D"].tolist() == D and got["nn"].tolist() == nn and got["keep"].tolist() == [bool(x) for x in keep]
        assert got["D"].dtype == np.int32 and got["nn"].dtype == np.int32 and got["keep"].dtype == bool
        assert got["info"]["kept"] == sum(keep) and got["info"]["keyed"] == sum(d >= 0 for d in D) and got["info"]["points"] == len(D)


def test_the_threshold_by_hand():
    five = hand_cases()[11]
    assert five[0] == "the threshold, alpha = 1"
    got = outliers_numpy(five[1], five[2], 1, 1.0, 0)
    assert got["sums"] == (5, 1536, 1179648) and got["info"]["mu"] == 307.2 and got["info"]["threshold"] == 683
    assert abs(got["info"]["sigma"] - math.sqrt(3538944) / 5) < 1e-12 and 1881 ** 2 < 3538944 < 1882 ** 2
    # the module's host arithmetic is the restatement's
    assert CO.threshold(5, 1536, 1179648, 1.0) == (got["info"]["mu"], got["info"]["sigma"], 683)
    assert CO.threshold(5, 1536, 1179648, 2.0)[2] == 1059 and CO.threshold(5, 1536, 1179648, 0.0)[2] == 307
    assert CO.threshold(5, 1536, 1179648, None)[2] is None
    assert CO.threshold(0, 0, 0, 2.0) == (0.0, 0.0, 0) and CO.threshold(1, 8192, 8192 ** 2, 2.0) == (8192.0, 0.0, 8192)
    # the largest sums: m = 2^31 - 1 points of D = 2^15 stay exact integers below 2^61 and 2^92
    m, d = (1 << 31) - 1, 1 << 15
    assert m * d * d < 1 << 61 and CO.threshold(m, m * d, m * d * d, 3.0) == (32768.0, 0.0, 32768)


def random_cloud(seed, n, grid=None):
    """n points over (and a little beyond) a 12 x 10 x 6 grid of 0.5 with clusters, exact duplicates and unkeyed points."""
    rng = np.random.default_rng(seed)
    g = grid or cloud.CloudGrid([10.0, 16.0, -3.0, 2.0, 0.0, 2.6], 0.5)
    lo, hi = np.array(g.border[0::2]), np.array(g.border[1::2])
    xyz = rng.uniform(lo - 0.2, hi + 0.2, (n, 3))
    c = rng.uniform(lo, hi, (3, 3))
    xyz[: n // 3] = c[rng.integers(0, 3, n // 3)] + rng.normal(0, 0.1, (n // 3, 3))
    xyz = xyz.astype(np.float32)
    xyz[rng.integers(0, n, n // 20)] = xyz[rng.integers(0, n, n // 20)]          # duplicates
    bad = rng.integers(0, n, max(n // 50, 1))
    xyz[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.float32([NAN, INF, -INF, 3e38]), len(bad))
    return xyz[rng.permutation(n)], g


@pytest.mark.parametrize("seed, n", [(0, 1), (1, 2), (2, 50), (3, 700), (4, 3000)])
def test_the_cell_list_is_the_brute_force(seed, n):
    xyz, g = random_cloud(seed, n)
    a, b = neighbours_numpy(xyz, g), neighbours_cells(xyz, g)
    ok = a[0]
    assert np.array_equal(ok, b[0]) and np.array_equal(a[1][ok], b[1][ok]) and np.array_equal(a[2][ok], b[2][ok])
    if n >= 700:
        assert 0 < (~ok).sum() < n // 4 and (a[1][ok][:, 0] == 0).any() and a[2][ok].max() > 40 and ((a[2][ok] < 8).any() or n > 1000)
        for k, alpha, m in ((1, 1.0, 0), (8, 1.0, 3), (32, None, 5)):
            w = outliers_from(a, k, alpha, m)
            assert 0 < w["info"]["kept"] < w["info"]["keyed"] and (w["D"][ok] <= CAP * k).all() and (w["D"][~ok] == -1).all()
            # the order of the points does not matter
            p = np.random.default_rng(n).permutation(n)
            wp = outliers_from(neighbours_cells(xyz[p], g), k, alpha, m)
            assert np.array_equal(wp["D"], w["D"][p]) and np.array_equal(wp["nn"], w["nn"][p]) and np.array_equal(wp["keep"], w["keep"][p])
            assert wp["sums"] == w["sums"] and wp["info"] == w["info"]


# ----------------------------------------------------------------------------------------
# settings and command lines
# ----------------------------------------------------------------------------------------
B6 = TC.B6


def test_settings_and_the_module_command_line(capsys, tmp_path):
    import argparse

    assert CO.check_settings({"radius": 1.5}) == (1.5, 8, 2.0, 0)
    assert CO.check_settings({"radius": 2, "k": 32, "alpha": None, "min_neighbours": 4, "border": B6}) == (2.0, 32, None, 4)
    assert CO.check_settings({"radius": 1.0, "k": None, "alpha": 0, "min_neighbours": None}) == (1.0, 8, 0.0, 0)
    good = {"radius": 1.0}
    for bad, msg in ((dict(good, radius=None), "radius"), (dict(good, radius=0.0), "radius"), (dict(good, radius=-1.0), "radius"),
                     (dict(good, radius=math.nan), "radius"), (dict(good, radius=math.inf), "radius"), (dict(good, radius="1"), "radius"),
                     (dict(good, k=0), " k "), (dict(good, k=33), " k "), (dict(good, k=2.5), " k "), (dict(good, k=True), " k "),
                     (dict(good, alpha=-0.5), "alpha"), (dict(good, alpha=math.nan), "alpha"), (dict(good, alpha=math.inf), "alpha"),
                     (dict(good, alpha="2"), "alpha"), (dict(good, min_neighbours=-1), "min_neighbours"),
                     (dict(good, min_neighbours=1 << 31), "min_neighbours"), (dict(good, min_neighbours=1.5), "min_neighbours"),
                     (dict(good, alpha=None), "at least one"), (dict(good, alpha=None, min_neighbours=0), "at least one"),
                     (dict(good, voxel=1.0), "unknown")):
        with pytest.raises(ValueError, match=msg):
            CO.check_settings(bad)
    with pytest.raises(ValueError, match="dict"):
        CO.check_settings(1.5)
    ap = argparse.ArgumentParser()
    CO.add_arguments(ap, prefix="o_")
    a = ap.parse_args(["--o_radius", "0.5"])
    assert CO.settings_from_args(a, prefix="o_") == {"radius": 0.5, "k": 8, "alpha": 2.0, "min_neighbours": 0} and CO.given(a, "o_") == []
    a = ap.parse_args(["--o_radius", "0.5", "--o_k=4", "--o_no_alpha", "--o_min_neighbours=3"])
    assert CO.settings_from_args(a, prefix="o_") == {"radius": 0.5, "k": 4, "alpha": None, "min_neighbours": 3}
    assert CO.given(a, "o_") == ["k", "min_neighbours", "no_alpha"]
    with pytest.raises(ValueError, match="exclude"):
        CO.settings_from_args(ap.parse_args(["--o_radius", "0.5", "--o_alpha=1", "--o_no_alpha"]), prefix="o_")
    src = cloud.write_cloud_ply(str(tmp_path / "in.ply"), np.zeros((2, 3), np.float32), None, None, np.ones(2, np.int32))
    base = ["--cloud", src, "--out", str(tmp_path / "out.ply")]
    full = base + ["--border=0,8,0,4,-1,1", "--radius=1"]
    for argv in (base, base + ["--border=0,8,0,4,-1,1"], base + ["--radius=1"], base + ["--border=0,8,0,4", "--radius=1"],
                 base + ["--border=0,8,0,4,-1,1", "--radius=0"], base + ["--border=0,8,0,4,-1,1", "--radius=1e-9"], full + ["--k=0"],
                 full + ["--k=33"], full + ["--alpha=-1"], full + ["--no_alpha"], full + ["--alpha=1", "--no_alpha", "--min_neighbours=2"],
                 full + ["--min_neighbours=-2"], ["--cloud", src, "--out", "out.xyz"] + full[4:], full[2:]):
        with pytest.raises(SystemExit):
            CO.main(argv)
    err = capsys.readouterr().err
    assert "--border is required" in err and "--radius is required" in err and ".ply" in err and "at least one" in err
    assert "exclude" in err and "2^21" in err and "min_neighbours" in err and " k " in err and "alpha" in err
    assert not (tmp_path / "out.ply").exists()


def test_cloud_settings_carry_the_outliers_and_keep_their_shape():
    good = {"path": "x.ply", "border": B6, "voxel": 0.5}
    grid, k = cloud.check_settings(dict(good, outliers={"radius": 1.5, "k": 4}))
    assert grid.n == (16, 8, 4) and k == 1
    assert cloud.check_settings(dict(good, outliers=None)) and cloud.check_settings(good)[1] == 1
    for bad, msg in ((1.5, "dict"), ({"radius": 0.0}, "radius"), ({"radius": 1.0, "k": 40}, " k "), ({"radius": 1e-7}, "2\\^21"),
                     ({"radius": 1.0, "alpha": None}, "at least one"), ({"k": 8}, "radius")):
        with pytest.raises(ValueError, match="cloud outliers.*" + msg):
            cloud.check_settings(dict(good, outliers=bad))
    import argparse

    ap = argparse.ArgumentParser()
    cloud.add_arguments(ap, prefix="c_")
    s = cloud.settings_from_args(ap.parse_args(["--c_border=0,8,0,4,-1,1", "--c_voxel", "0.5"]), "x.ply", prefix="c_")
    assert sorted(s) == ["border", "min_points", "path", "voxel"]
    assert "statistical" not in cloud.__doc__.split("Out of scope")[1]


def test_predict_flags_and_their_errors(capsys):
    base = ["--output_folder", "o", "--fuse", "--cloud", "c.ply", "--cloud_voxel=0.5", "--cloud_border=0,8,0,4,-1,1"]
    a = predict.parse_args(base)
    assert a.cloud_outlier_radius is None and "outliers" not in predict._cloud_settings(a)
    assert sorted(predict._cloud_settings(a)) == ["border", "min_points", "path", "voxel"]
    s = predict._cloud_settings(predict.parse_args(base + ["--cloud_outlier_radius=1.5"]))
    assert s["outliers"] == {"radius": 1.5, "k": 8, "alpha": 2.0, "min_neighbours": 0} and s["voxel"] == 0.5
    s = predict._cloud_settings(predict.parse_args(base + ["--cloud_outlier_radius=1.5", "--cloud_outlier_k=16", "--cloud_outlier_alpha=1",
                                                           "--cloud_outlier_min_neighbours=2"]))
    assert s["outliers"] == {"radius": 1.5, "k": 16, "alpha": 1.0, "min_neighbours": 2}
    s = predict._cloud_settings(predict.parse_args(base + ["--cloud_outlier_radius=1.5", "--cloud_outlier_no_alpha", "--cloud_outlier_min_neighbours=2"]))
    assert s["outliers"]["alpha"] is None
    for argv in (base + ["--cloud_outlier_k=4"], base + ["--cloud_outlier_alpha=1"], base + ["--cloud_outlier_min_neighbours=2"],
                 base + ["--cloud_outlier_radius=0"], base + ["--cloud_outlier_radius=1", "--cloud_outlier_k=33"],
                 base + ["--cloud_outlier_radius=1", "--cloud_outlier_alpha=-2"], base + ["--cloud_outlier_radius=1e-9"],
                 base + ["--cloud_outlier_radius=1", "--cloud_outlier_no_alpha"], base[:3] + ["--cloud_outlier_radius=1"]):
        with pytest.raises(SystemExit):
            predict.parse_args(argv)
    err = capsys.readouterr().err
    for flag in ("--cloud_outlier_k needs --cloud_outlier_radius", "--cloud_outlier_alpha needs", "--cloud_outlier_min_neighbours needs",
                 "--cloud_outlier_radius needs --cloud", "radius must be finite", " k ", "alpha", "2^21", "at least one"):
        assert flag in err, flag


def test_pipeline_validates_the_outlier_settings_up_front():
    good = {"path": "c.ply", "border": B6, "voxel": 0.5}
    # every error below is raised before the model or the dataset is touched
    for bad, msg in (({"radius": -1.0}, "radius"), ({"radius": 1.0, "k": 0}, " k "), ({"radius": 1.0, "alpha": -1.0}, "alpha"),
                     ({"radius": 1.0, "min_neighbours": -1}, "min_neighbours"), ({"radius": 1.0, "alpha": None}, "at least one"),
                     ({"radius": 1e-7}, "2\\^21"), ("1.0", "dict"), ({"radius": 1.0, "path": "x"}, "unknown")):
        with pytest.raises(ValueError, match=msg):
            pipeline.predict_and_fuse(None, None, "unused", cloud=dict(good, outliers=bad))
    import inspect

    assert list(inspect.signature(pipeline.predict_and_fuse).parameters)[-1] == "cloud"


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
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    lib = _lib.load()
    assert lib.d3d_build_flags() == b""
    assert lib.d3d_cloud_outliers_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_cloud_outliers_scratch_bytes(0) > 0
    assert lib.d3d_cloud_outliers_scratch_bytes(1_000_000) >= 16 * 1_000_000
    assert lib.d3d_cloud_outliers_scratch_bytes((1 << 31) - 1) >= 16 * ((1 << 31) - 1)
    for bad in (-1, 1 << 31):
        assert lib.d3d_cloud_outliers_scratch_bytes(bad) == 0, bad


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    need = lib.d3d_cloud_outliers_scratch_bytes(10)
    ok = dict(xyz=P(1), keys=P(2), order=P(3), n=10, nx=16, ny=8, nz=4, h=0.5, k=8, s=P(4), sb=need, dist=P(5), nn=P(6), sums=P(7), st=None)
    order = ["xyz", "keys", "order", "n", "nx", "ny", "nz", "h", "k", "s", "sb", "dist", "nn", "sums", "st"]
    TC._expect(lib, lib.d3d_cloud_outliers_distances, ok, order,
               [(dict([(name, None)]), b"null") for name in ("xyz", "keys", "order", "s", "dist", "nn", "sums")] +
               [(dict(n=-1), b"n_points"), (dict(n=1 << 31), b"n_points"), (dict(nx=0), b"grid"), (dict(ny=1 << 21), b"grid"), (dict(nz=-3), b"grid"),
                (dict(h=0.0), b"radius"), (dict(h=-1.0), b"radius"), (dict(h=math.nan), b"radius"), (dict(h=math.inf), b"radius"),
                (dict(k=0), b"k="), (dict(k=33), b"k="), (dict(k=-4), b"k="), (dict(sb=need - 1), b"scratch"), (dict(sb=0), b"scratch"),
                (dict(nn=P(5)), b"alias"), (dict(dist=ctypes.c_void_p((1 << 32) + 119)), b"alias"), (dict(sums=ctypes.c_void_p((4 << 32) + need - 1)), b"alias"),
                (dict(sums=ctypes.c_void_p((6 << 32) + 36)), b"alias"), (dict(order=ctypes.c_void_p((2 << 32) + 72)), b"alias"),
                (dict(dist=ctypes.c_void_p((7 << 32) + 16)), b"alias")])
    # what is not an error: no points -- and nothing is launched or written for them
    assert lib.d3d_cloud_outliers_distances(None, None, None, 0, 16, 8, 4, 0.5, 8, P(4), need, None, None, P(7), None) == 0
    assert lib.d3d_cloud_outliers_distances(None, None, None, 0, 16, 8, 4, 0.5, 8, None, need, None, None, P(7), None) == -1


def test_the_operator_refuses_cpu_tensors_bad_dtypes_and_settings():
    g = TC.unit_grid()
    xyz = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CO.point_distances(xyz, g, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CO.outlier_mask(xyz, g.border, 1.0)
    c = {"xyz": xyz, "normal": None, "color": None, "count": torch.ones(5, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CO.filter_cloud(c, {"radius": 1.0}, g.border)
    for bad in (xyz.double(), torch.zeros(5, 2), torch.zeros(15)):
        with pytest.raises(ValueError, match="xyz"):
            CO.point_distances(bad, g, 8)
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match=" k "):
            CO.point_distances(xyz, g, k)
    with pytest.raises(TypeError, match="CloudGrid"):
        CO.point_distances(xyz, [0, 4, 0, 4, 0, 4], 8)
    with pytest.raises(TypeError, match="Tensor"):
        CO.point_distances(np.zeros((5, 3), np.float32), g, 8)
    for kw, msg in ((dict(alpha=None), "at least one"), (dict(alpha=-1.0), "alpha"), (dict(min_neighbours=-1), "min_neighbours"),
                    (dict(k=0), " k "), (dict(radius=0.0), "voxel"), (dict(radius=1e-9), "2\\^21"), (dict(border=[0, 4, 0, 4]), "six")):
        with pytest.raises(ValueError, match=msg):
            CO.outlier_mask(**dict(dict(xyz=xyz, border=g.border, radius=1.0), **kw))
    with pytest.raises(ValueError, match="border"):
        CO.filter_cloud(c, {"radius": 1.0})
    with pytest.raises(ValueError, match="merge_points"):
        CO.filter_cloud({"xyz": xyz}, {"radius": 1.0}, g.border)
    with pytest.raises(ValueError, match="count"):
        CO.filter_cloud(dict(c, count=torch.ones(4, dtype=torch.int32)), {"radius": 1.0}, g.border)


def test_the_kernels_use_integer_atomic_add_only_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/cloud_outliers.hip").read())
    assert set(re.findall(r"\batomic\w*", hip)) == {"atomicAdd"}
    assert not re.search(r"unsafeAtomic|atomicAdd\s*\(\s*\(?\s*(float|double)\s*\*|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
    # one atomicAdd, a statement (its result is not used), on the unsigned 64-bit sums
    assert len(re.findall(r"(?:^|[;{}\)])\s*atomicAdd\(", hip, re.M)) == len(re.findall(r"\batomicAdd\(", hip)) == 1
    assert re.search(r"unsigned long long\* __restrict__ sums\)", hip) and "atomicAdd(sums + threadIdx.x, (unsigned long long)t)" in hip
    assert "fma" not in hip
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bcloud_outliers\.hip\b", make, re.M) and "-ffp-contract=off" in make
    assert "ifeq ($(CLOUD_OUTLIERS),plain)" in make and "-DD3D_CLOUD_OUTLIERS_PLAIN" in make
