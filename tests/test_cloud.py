"""CPU checks of the merged point cloud (deep3d_aerial_amd/cloud.py, csrc/cloud.hip).  `cloud_numpy` restates
the rule of cloud.py's docstring in numpy -- no fused multiply-add, one look-up per neighbour instead of the kernels' runs of
keys -- and is checked here against hand-computed answers; tests/test_cloud_gpu.py compares the kernels against it bit for bit.
Also: the PLY round trip, the settings, both command lines, the pipeline's up-front validation, the C ABI and its argument checks,
and the operator's refusals."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from deep3d_aerial_amd import _lib, cloud, pipeline, predict

NEW_SYMBOLS = ("d3d_cloud_scratch_bytes", "d3d_cloud_keys", "d3d_cloud_heads", "d3d_cloud_accumulate", "d3d_cloud_neighbours",
               "d3d_cloud_finalize")
M = (1 << 21) - 2   # the largest voxel index of the largest grid


# ----------------------------------------------------------------------------------------
# numpy restatement
# ----------------------------------------------------------------------------------------
def cells_numpy(xyz, grid):
    """(ok [n] bool, i [n,3] int64, r [n,3] int64) of every point; i and r are 0 where the point is dropped."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    lo = np.array(grid.border[0::2], np.float64)
    nn = np.array(grid.n, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x.astype(np.float64) - lo) / np.float64(grid.voxel)
        fi = np.floor(u)
        ok = np.isfinite(x).all(1) & ((fi >= 0) & (fi <= nn - 1)).all(1)
        fr = np.floor((u - fi) * 65536.0)
    i = np.where(ok[:, None], fi, 0.0).astype(np.int64)
    r = np.where(ok[:, None], fr, 0.0).astype(np.int64)
    return ok, i, r


def keys_numpy(xyz, grid):
    ok, i, _ = cells_numpy(xyz, grid)
    return np.where(ok, (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0], np.iinfo(np.int64).max)


def cloud_numpy(xyz, normal, color, grid, min_points=1):
    """{"xyz", "normal" | None, "color" | None, "count", "key", "kept"} as cloud.py's docstring states them; "key" are the kept
    voxels' keys and "kept" the flags over all occupied voxels (in key order)."""
    ok, i, r = cells_numpy(xyz, grid)
    key = ((i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0])[ok]
    ukeys, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    m = len(ukeys)
    count = np.bincount(inv, minlength=m).astype(np.int64)
    S = np.zeros((m, 3), np.int64)
    np.add.at(S, inv, r[ok])
    iu = np.stack([ukeys & ((1 << 21) - 1), (ukeys >> 21) & ((1 << 21) - 1), ukeys >> 42], 1)
    lo = np.array(grid.border[0::2], np.float64)
    v = np.float64(grid.voxel)
    cd = count.astype(np.float64)[:, None]
    q = (S.astype(np.float64) + 0.5 * cd) / (65536.0 * cd)
    t = iu.astype(np.float64) + q
    t = t * v                                   # a product, rounded
    out_xyz = (lo + t).astype(np.float32)       # then a sum, rounded: no fma
    out_n = out_c = None
    if normal is not None:
        nr = np.asarray(normal, np.float32).reshape(-1, 3)[ok]
        with np.errstate(invalid="ignore"):
            use = (np.abs(nr) <= np.float32(1024.0)).all(1)   # false for a NaN, false for an Inf
        nq = np.where(use[:, None], np.rint(np.where(use[:, None], nr, 0).astype(np.float64) * 1048576.0), 0.0).astype(np.int64)
        N = np.zeros((m, 3), np.int64)
        np.add.at(N, inv, nq)
        x, y, z = (N[:, k].astype(np.float64) for k in range(3))
        ln = np.sqrt((x * x + y * y) + z * z)
        zero = (N == 0).all(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out_n = np.where(zero[:, None], 0.0, np.stack([x, y, z], 1) / np.where(zero, 1.0, ln)[:, None]).astype(np.float32)
    if color is not None:
        c = np.clip(np.asarray(color, np.int64).reshape(-1, 3), 0, 255)[ok]
        C = np.zeros((m, 3), np.int64)
        np.add.at(C, inv, c)
        out_c = ((2 * C + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    total = np.zeros(m, np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nb = iu + np.array([dx, dy, dz], np.int64)
                inside = ((nb >= 0) & (nb < np.array(grid.n, np.int64))).all(1)
                nk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
                at = np.minimum(np.searchsorted(ukeys, nk), max(m - 1, 0))
                hit = inside & (ukeys[at] == nk) if m else inside
                total += np.where(hit, count[at], 0) if m else 0
    kept = total >= int(min_points)
    pick = lambda a: None if a is None else np.ascontiguousarray(a[kept])
    return {"xyz": pick(out_xyz), "normal": pick(out_n), "color": pick(out_c), "count": count[kept].astype(np.int32), "key": ukeys[kept],
            "kept": kept}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_cloud(got, want):
    """Two cloud dicts (host arrays) equal bit for bit in every output array."""
    assert got["xyz"].shape == want["xyz"].shape and np.array_equal(bits(got["xyz"]), bits(want["xyz"]))
    assert np.array_equal(got["count"], want["count"]) and got["count"].dtype == np.int32
    for k in ("normal", "color"):
        assert (got[k] is None) == (want[k] is None), k
    if want["normal"] is not None:
        assert np.array_equal(bits(got["normal"]), bits(want["normal"]))
    if want["color"] is not None:
        assert got["color"].dtype == np.uint8 and np.array_equal(got["color"], want["color"])


# ----------------------------------------------------------------------------------------
# crafted cases (shared with tests/test_cloud_gpu.py): (name, xyz, normal, color, grid, min_points)
# ----------------------------------------------------------------------------------------
def unit_grid(nx=4, ny=4, nz=4):
    return cloud.CloudGrid([0.0, nx, 0.0, ny, 0.0, nz], 1.0)


def big_grid():
    """2^21 - 1 voxels of 2^-10 per axis: the largest grid."""
    v = 2.0 ** -10
    hi = ((1 << 21) - 1) * v
    return cloud.CloudGrid([0.0, hi, 0.0, hi, 0.0, hi], v)


def tie_case():
    xyz = np.float32([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5]])
    return xyz, np.float32([[0, 0, 1], [0, 0, 1]]), np.int32([[10, 0, 255], [11, 1, 255]]), unit_grid()


def faces_case():
    """A point on each min face and inside (kept), then one on each max face with integer u (dropped)."""
    xyz = np.float32([[0, 1.5, 1.5], [1.5, 0, 1.5], [1.5, 1.5, 0], [0, 0, 0], [4, 1.5, 1.5], [1.5, 4, 1.5], [1.5, 1.5, 4], [4, 4, 4]])
    return xyz, None, None, unit_grid()


def packing_case():
    v = 2.0 ** -10
    c = np.float32((M + 0.5) * v)
    assert float(c) == (M + 0.5) * v   # exact in fp32
    h = np.float32(0.5 * v)
    xyz = np.float32([[c, h, h], [h, c, h], [h, h, c]])
    return xyz, None, np.int32([[1, 2, 3], [4, 5, 6], [7, 8, 9]]), big_grid()


def filter_case():
    """Voxels of a 4 x 3 x 3 grid: A = (3,0,0) x 5, B = (0,1,0) x 1, D = (0,2,2) x 1, E = (3,2,2) x 2, G1 = (2,0,2) x 1,
    G2 = (3,0,2) x 1.  A is the last voxel of row (y 0, z 0), B the first of the next row."""
    g = unit_grid(4, 3, 3)
    vox = [(3, 0, 0)] * 5 + [(0, 1, 0)] + [(0, 2, 2)] + [(3, 2, 2)] * 2 + [(2, 0, 2)] + [(3, 0, 2)]
    rng = np.random.default_rng(5)
    xyz = (np.array(vox, np.float64) + rng.uniform(0.1, 0.9, (len(vox), 3))).astype(np.float32)
    return xyz, None, None, g


def key_of(ix, iy, iz):
    return (iz << 42) | (iy << 21) | ix


# ----------------------------------------------------------------------------------------
# the rule, by hand
# ----------------------------------------------------------------------------------------
def test_a_colour_tie_rounds_up_and_the_position_is_the_mean_of_the_cell_centres():
    xyz, nrm, col, g = tie_case()
    c = cloud_numpy(xyz, nrm, col, g)
    assert c["count"].tolist() == [2] and c["key"].tolist() == [0]
    assert c["color"].tolist() == [[11, 1, 255]]          # 10.5 -> 11, 0.5 -> 1
    # r = 32768 and 49152: (81920 + 1) / 131072
    assert c["xyz"].dtype == np.float32 and c["xyz"][0, 0] == np.float32(81921.0 / 131072.0)
    assert c["xyz"][0, 1] == np.float32(65537.0 / 131072.0) and c["xyz"][0, 2] == c["xyz"][0, 1]
    assert c["normal"].tolist() == [[0.0, 0.0, 1.0]]
    # out-of-range colours are clamped on input
    c = cloud_numpy(xyz, None, np.int32([[-5, 300, 255], [0, 255, 256]]), g)
    assert c["color"].tolist() == [[0, 255, 255]] and c["normal"] is None


def test_min_faces_are_kept_and_max_faces_with_an_integer_u_are_dropped():
    xyz, _, _, g = faces_case()
    c = cloud_numpy(xyz, None, None, g)
    assert c["key"].tolist() == sorted([key_of(0, 1, 1), key_of(1, 0, 1), key_of(1, 1, 0), 0]) and c["count"].tolist() == [1, 1, 1, 1]
    assert (keys_numpy(xyz, g)[4:] == np.iinfo(np.int64).max).all()
    # a border that is no multiple of the voxel: the last voxel is cut, and its max face (u = 3.5) lies inside it
    g2 = cloud.CloudGrid([0.0, 3.5, 0.0, 1.0, 0.0, 1.0], 1.0)
    assert g2.n == (4, 1, 1)
    c = cloud_numpy(np.float32([[3.5, 0.5, 0.5], [3.99, 0.5, 0.5], [4.0, 0.5, 0.5]]), None, None, g2)
    assert c["key"].tolist() == [3] and c["count"].tolist() == [2]


def test_nan_and_inf_are_dropped_and_minus_zero_is_zero():
    g = unit_grid()
    xyz = np.float32([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1.5, 1.5, 1.5], [-1e-30, 1, 1], [3e38, 1, 1]])
    c = cloud_numpy(xyz, None, None, g)
    assert c["key"].tolist() == [key_of(1, 1, 1)] and c["count"].tolist() == [1]
    a = cloud_numpy(np.float32([[-0.0, -0.0, -0.0], [0.25, 0.5, -0.0]]), None, None, g)
    b = cloud_numpy(np.float32([[0.0, 0.0, 0.0], [0.25, 0.5, 0.0]]), None, None, g)
    same_cloud(a, b)
    assert a["key"].tolist() == [0] and a["count"].tolist() == [2]
    assert a["xyz"][0].tolist() == [np.float32((16384 + 1.0) / 131072.0), np.float32((32768 + 1.0) / 131072.0), np.float32(1.0 / 131072.0)]
    # no point at all, and only dropped points
    for pts in (np.zeros((0, 3), np.float32), xyz[:3]):
        c = cloud_numpy(pts, pts, np.zeros(pts.shape, np.int32), g)
        assert c["xyz"].shape == (0, 3) and c["normal"].shape == (0, 3) and c["color"].shape == (0, 3) and c["count"].shape == (0,)


def test_a_nan_normal_adds_nothing_and_opposite_normals_cancel():
    g = unit_grid()
    xyz = np.float32([[0.5, 0.5, 0.5]] * 2 + [[1.5, 0.5, 0.5]] * 2 + [[2.5, 0.5, 0.5]] * 2 + [[3.5, 0.5, 0.5]])
    nrm = np.float32([[np.nan, 0, 1], [0, 0, 1], [0.6, 0, 0.8], [-0.6, 0, -0.8], [np.inf, 0, 0], [0, 2e3, 0], [3, 0, 4]])
    c = cloud_numpy(xyz, nrm, None, g)
    assert c["normal"].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0], [np.float32(0.6), 0, np.float32(0.8)]]
    assert c["count"].tolist() == [2, 2, 2, 1]


def test_the_key_packs_three_fields_of_21_bits():
    xyz, _, col, g = packing_case()
    assert g.n == (M + 1, M + 1, M + 1)
    assert keys_numpy(xyz, g).tolist() == [M, M << 21, M << 42]
    c = cloud_numpy(xyz, None, col, g)
    assert c["key"].tolist() == [M, M << 21, M << 42] and c["color"].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    # every point sits on a cell centre: r = 32768, the output is the input up to the half 65536th
    assert np.abs(c["xyz"].astype(np.float64) - xyz.astype(np.float64)).max() <= g.voxel / 65536 + float(np.spacing(np.float32(2048)))
    for bad in (2.0 ** -10 * (1 << 21), 1e9):
        with pytest.raises(ValueError, match="2\\^21"):
            cloud.CloudGrid([0.0, bad, 0.0, 1.0, 0.0, 1.0], 2.0 ** -10)


def test_the_isolated_voxel_filter_at_the_borders_and_across_rows():
    xyz, _, _, g = filter_case()
    A, B, D, E, G1, G2 = key_of(3, 0, 0), key_of(0, 1, 0), key_of(0, 2, 2), key_of(3, 2, 2), key_of(2, 0, 2), key_of(3, 0, 2)
    c = cloud_numpy(xyz, None, None, g, 1)
    assert c["key"].tolist() == sorted([A, B, D, E, G1, G2]) == [A, B, G1, G2, D, E] and c["count"].tolist() == [5, 1, 1, 1, 1, 2]
    # K = 2: B sees only itself (A, full, is the last voxel of the previous row: x = 3 is no neighbour of x = 0); D likewise
    assert cloud_numpy(xyz, None, None, g, 2)["key"].tolist() == [A, G1, G2, E]
    assert cloud_numpy(xyz, None, None, g, 3)["key"].tolist() == [A]
    assert cloud_numpy(xyz, None, None, g, 5)["key"].tolist() == [A]
    assert cloud_numpy(xyz, None, None, g, 6)["key"].tolist() == []
    # one pass: a chain of three single points with K = 3 keeps its middle, whose neighbours have gone
    g1 = cloud.CloudGrid([0.0, 5.0, 0.0, 1.0, 0.0, 1.0], 1.0)
    c = cloud_numpy(np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]]), None, None, g1, 3)
    assert c["key"].tolist() == [1] and c["count"].tolist() == [1]
    # the same at the far corner of the largest grid: (M, M, M) and its neighbour (M - 1, M, M)
    gb = big_grid()
    v = gb.voxel
    c0, c1 = np.float32((M + 0.5) * v), np.float32((M - 0.5) * v)
    pts = np.float32([[c0, c0, c0], [c1, c0, c0], [np.float32(0.5 * v), c0, c0]])
    assert cloud_numpy(pts, None, None, gb, 2)["key"].tolist() == [key_of(M - 1, M, M), key_of(M, M, M)]


def test_the_position_is_within_a_65536th_of_a_voxel_and_one_ulp_of_the_float64_mean():
    rng = np.random.default_rng(11)
    g = cloud.CloudGrid([100.0, 103.7, -50.0, -46.3, 5.0, 6.11], 0.37)   # 10 x 10 x 3 voxels, the last layer cut
    xyz = (np.array([100.0, -50.0, 5.0]) + rng.uniform(0, 1, (10000, 3)) * np.array([3.7, 3.7, 1.11])).astype(np.float32)
    xyz = xyz[cells_numpy(xyz, g)[0]]   # (a point that fp32 rounds onto a max face is dropped by the rule)
    c = cloud_numpy(xyz, None, None, g)
    ok, i, _ = cells_numpy(xyz, g)
    assert ok.all()
    key = (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]
    uk, inv = np.unique(key, return_inverse=True)
    mean = np.zeros((len(uk), 3))
    np.add.at(mean, inv.reshape(-1), xyz.astype(np.float64))
    mean /= np.bincount(inv.reshape(-1))[:, None]
    assert np.array_equal(uk, c["key"]) and 2 < c["count"].mean() < 50
    err = np.abs(c["xyz"].astype(np.float64) - mean)
    bound = g.voxel / 65536 + np.spacing(np.abs(c["xyz"])).astype(np.float64)
    assert (err <= bound).all(), float((err / bound).max())
    # and the order of the points does not matter
    p = rng.permutation(len(xyz))
    same_cloud(cloud_numpy(xyz[p], None, None, g), c)


# ----------------------------------------------------------------------------------------
# the file
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("colors", [False, True])
def test_ply_round_trip(tmp_path, normals, colors):
    rng = np.random.default_rng(3)
    m = 17
    xyz = rng.normal(size=(m, 3)).astype(np.float32)
    nrm = rng.normal(size=(m, 3)).astype(np.float32) if normals else None
    col = rng.integers(0, 256, (m, 3)).astype(np.uint8) if colors else None
    cnt = rng.integers(1, 1000, m).astype(np.int32)
    path = cloud.write_cloud_ply(str(tmp_path / "sub" / "c.ply"), torch.from_numpy(xyz), nrm, col, cnt)
    data = open(path, "rb").read()
    assert data == cloud.cloud_ply_bytes(xyz, nrm, col, cnt)
    head = data[:data.index(b"end_header\n")].decode().split("\n")
    want = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue"] if colors else []) + ["count"]
    assert [ln.split()[2] for ln in head if ln.startswith("property")] == want
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 17" in head
    assert len(data) - data.index(b"end_header\n") - 11 == m * (12 + 12 * normals + 3 * colors + 4)
    back = cloud.read_cloud_ply(path)
    same_cloud(back, {"xyz": xyz, "normal": nrm, "color": col, "count": cnt})
    assert cloud.cloud_ply_bytes(back["xyz"], back["normal"], back["color"], back["count"]) == data
    # an empty cloud
    e = cloud.read_cloud_ply(cloud.write_cloud_ply(str(tmp_path / "e.ply"), xyz[:0], None if nrm is None else nrm[:0],
                                                   None if col is None else col[:0], cnt[:0]))
    assert e["xyz"].shape == (0, 3) and e["count"].shape == (0,) and (e["normal"] is None) == (not normals)
    with pytest.raises(ValueError):
        cloud.cloud_ply_bytes(xyz, nrm, col, cnt.astype(np.int64))
    (tmp_path / "bad.ply").write_bytes(data[:-1])
    with pytest.raises(ValueError, match="bytes"):
        cloud.read_cloud_ply(str(tmp_path / "bad.ply"))


# ----------------------------------------------------------------------------------------
# settings and command lines
# ----------------------------------------------------------------------------------------
B6 = [0.0, 8.0, 0.0, 4.0, -1.0, 1.0]


def test_settings_and_the_module_command_line(capsys, tmp_path):
    import argparse

    ap = argparse.ArgumentParser()
    cloud.add_arguments(ap, prefix="c_")
    a = ap.parse_args(["--c_border=0,8,0,4,-1,1", "--c_voxel", "0.5", "--c_min_points", "3"])
    s = cloud.settings_from_args(a, "x.ply", prefix="c_")
    assert s == {"path": "x.ply", "border": B6, "voxel": 0.5, "min_points": 3}
    grid, k = cloud.check_settings(s)
    assert grid.n == (16, 8, 4) and k == 3 and grid.border == B6 and grid.voxel == 0.5
    assert cloud.check_settings({"path": "x.ply", "border": B6, "voxel": 1})[1] == 1
    good = {"path": "x.ply", "border": B6, "voxel": 0.5}
    for bad, msg in ((dict(good, path="x.tif"), ".ply"), (dict(good, path=None), ".ply"), (dict(good, border=None), "border"),
                     (dict(good, border=[0, 8, 0, 4]), "six"), (dict(good, border=[0, 8, 0, 4, 1, 1]), "below"),
                     (dict(good, border=[0, math.inf, 0, 4, 0, 1]), "finite"), (dict(good, voxel=None), "voxel"),
                     (dict(good, voxel=0.0), "voxel"), (dict(good, voxel=math.nan), "voxel"), (dict(good, voxel=1e-9), "2\\^21"),
                     (dict(good, min_points=0), "min_points"), (dict(good, min_points=2.5), "min_points"),
                     (dict(good, min_points=True), "min_points"), (dict(good, min_points=1 << 31), "min_points")):
        with pytest.raises(ValueError, match=msg):
            cloud.check_settings(bad)
    with pytest.raises(ValueError, match="dict"):
        cloud.check_settings("x.ply")
    base = ["--fused", str(tmp_path), "--out", str(tmp_path / "c.ply")]
    for argv in (base, base + ["--border=0,8,0,4,-1,1"], base + ["--voxel=1"], base + ["--border=0,8,0,4", "--voxel=1"],
                 base + ["--border=0,8,0,4,-1,1", "--voxel=0"], base + ["--border=0,8,0,4,-1,1", "--voxel=1", "--min_points=0"],
                 ["--fused", str(tmp_path), "--out", "c.xyz", "--border=0,8,0,4,-1,1", "--voxel=1"]):
        with pytest.raises(SystemExit):
            cloud.main(argv)
    err = capsys.readouterr().err
    assert "--border is required" in err and "--voxel is required" in err and ".ply" in err and "min_points" in err
    assert not (tmp_path / "c.ply").exists()


def test_read_fused_reads_what_save_fused_writes(tmp_path):
    def result(ref, n, scene=None):
        pts = {"xyz": torch.full((n, 3), float(len(ref))), "normal": torch.ones((n, 3)), "views": torch.zeros((n, 2), dtype=torch.int32),
               "nviews": torch.zeros((n,), dtype=torch.int32), "n_valid": n, "color": None}
        r = {"ref": ref, "final_mask": torch.zeros((4, 8), dtype=torch.bool), "points": pts}
        return dict(r, scene=scene) if scene is not None else r

    pipeline.save_fused([result("bb", 3), result("a", 2), result("ccc", 0)], str(tmp_path / "f"))
    xyz, nrm = cloud.read_fused(str(tmp_path / "f"))
    assert xyz[:, 0].tolist() == [1, 1, 2, 2, 2] and nrm.shape == (5, 3) and xyz.dtype == np.float32
    pipeline.save_fused([result("a", 2, scene=1), result("a", 1, scene=0)], str(tmp_path / "g"))
    assert cloud.read_fused(str(tmp_path / "g"))[0].shape == (3, 3)
    with pytest.raises(FileNotFoundError):
        cloud.read_fused(str(tmp_path / "none"))


def test_predict_flags_and_their_defaults(capsys):
    base = ["--output_folder", "o", "--fuse"]
    a = predict.parse_args(base)
    assert a.cloud is None
    s = predict._cloud_settings(predict.parse_args(base + ["--cloud", "c.ply", "--cloud_voxel=0.5", "--cloud_border=0,8,0,4,-1,1"]))
    assert s == {"path": "c.ply", "border": B6, "voxel": 0.5, "min_points": 1}
    # the border: the mesh's box first, then a DSM border with Z bounds
    mesh = ["--mesh", "m.ply", "--mesh_border=0,2,0,2,0,2", "--mesh_voxel=0.1"]
    s = predict._cloud_settings(predict.parse_args(base + mesh + ["--cloud", "c.ply", "--cloud_voxel=0.5", "--cloud_min_points=4",
                                                                  "--dsm_border=0,8,0,4,-1,1"]))
    assert s == {"path": "c.ply", "border": [0.0, 2.0, 0.0, 2.0, 0.0, 2.0], "voxel": 0.5, "min_points": 4}
    s = predict._cloud_settings(predict.parse_args(base + ["--cloud", "c.ply", "--cloud_voxel=0.5", "--dsm_border=0,8,0,4,-1,1"]))
    assert s["border"] == B6
    for argv in (base + ["--cloud", "c.ply", "--cloud_voxel=0.5"], base + ["--cloud", "c.ply", "--cloud_voxel=0.5", "--dsm_border=0,8,0,4"],
                 base + ["--cloud", "c.ply", "--cloud_border=0,8,0,4,-1,1"], base + ["--cloud", "c.xyz", "--cloud_voxel=1", "--cloud_border=0,8,0,4,-1,1"],
                 base + ["--cloud", "c.ply", "--cloud_voxel=0", "--cloud_border=0,8,0,4,-1,1"],
                 base + ["--cloud", "c.ply", "--cloud_voxel=1", "--cloud_border=0,8,0,4"],
                 base + ["--cloud", "c.ply", "--cloud_voxel=1", "--cloud_border=0,8,0,4,-1,1", "--cloud_min_points=0"],
                 base + ["--cloud", "c.ply", "--cloud_voxel=1", "--cloud_border=0,8,0,4,-1,1", "--fuse_partition", "scene_blocks"],
                 base[:2] + ["--cloud", "c.ply", "--cloud_voxel=1", "--cloud_border=0,8,0,4,-1,1"]):
        with pytest.raises(SystemExit):
            predict.parse_args(argv)
    err = capsys.readouterr().err
    assert "--cloud needs --fuse" in err and "--cloud needs --cloud_border" in err and "--cloud needs --cloud_voxel" in err
    assert ".ply" in err and "min_points" in err and "--fuse_partition views" in err


def test_pipeline_validates_the_cloud_settings_up_front():
    good = {"path": "c.ply", "border": B6, "voxel": 0.5}
    # every error below is raised before the model or the dataset is touched
    for bad, msg in ((dict(good, path="c.tif"), ".ply"), (dict(good, border=None), "border"), (dict(good, border=B6[:4]), "six"),
                     (dict(good, voxel=-1.0), "voxel"), (dict(good, voxel=1e-7), "2\\^21"), (dict(good, min_points=0), "min_points"),
                     ("c.ply", "dict")):
        with pytest.raises(ValueError, match=msg):
            pipeline.predict_and_fuse(None, None, "unused", cloud=bad)
    with pytest.raises(ValueError, match="scene_blocks"):
        pipeline.predict_and_fuse(None, None, "unused", world_size=2, fuse_partition="scene_blocks", cloud=good)
    import inspect

    assert list(inspect.signature(pipeline.predict_and_fuse).parameters)[-1] == "cloud"


def test_reference_colors():
    im = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1)
    c = pipeline.reference_colors(im, 16, 16)
    assert tuple(c.shape) == (16, 16, 3) and c.dtype == torch.float32 and c.is_contiguous()
    # the gather kernel's int(c * 255.0f) returns every byte
    assert torch.equal((c * torch.tensor(255.0)).to(torch.int32)[:, :, 1].reshape(-1), torch.arange(256, dtype=torch.int32))
    rgb = torch.zeros((4, 6, 3), dtype=torch.uint8)
    assert tuple(pipeline.reference_colors(rgb, 4, 6).shape) == (4, 6, 3)
    for bad, msg in ((rgb, "4 x 6"), (rgb.float(), "uint8"), (torch.zeros((4, 6, 4), dtype=torch.uint8), "uint8")):
        with pytest.raises(ValueError, match=msg):
            pipeline.reference_colors(bad, 6, 4)


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
    assert lib.d3d_cloud_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_cloud_scratch_bytes(0) > 0
    assert lib.d3d_cloud_scratch_bytes(1_000_000) >= 4 * 1_000_000 + 8 * math.ceil(1_000_000 / 4096)
    assert lib.d3d_cloud_scratch_bytes((1 << 31) - 1) >= 4 * ((1 << 31) - 1)
    for bad in (-1, 1 << 31):
        assert lib.d3d_cloud_scratch_bytes(bad) == 0, bad


def _expect(lib, fn, ok, order, cases):
    for kw, msg in cases:
        a = dict(ok, **kw)
        assert fn(*[a[k] for k in order]) == -1, kw
        assert msg in lib.d3d_last_error(), (kw, lib.d3d_last_error())


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    inf, nan = math.inf, math.nan
    grid = dict(x0=0.0, x1=8.0, y0=0.0, y1=4.0, z0=-1.0, z1=1.0, v=0.5)
    grid_order = ["x0", "x1", "y0", "y1", "z0", "z1", "v"]
    grid_cases = [(dict(x0=nan), b"finite"), (dict(y1=inf), b"finite"), (dict(z0=1.0), b"below"), (dict(x1=0.0), b"below"),
                  (dict(v=0.0), b"voxel"), (dict(v=-1.0), b"voxel"), (dict(v=nan), b"voxel"), (dict(v=inf), b"voxel"),
                  (dict(v=1e-6), b"grid"), (dict(x1=3e6, v=1.0), b"grid")]
    bad_n = lambda name: [(dict([(name, -1)]), b"n_"), (dict([(name, 1 << 31)]), b"n_")]
    # keys
    ok = dict(grid, xyz=P(1), n=10, keys=P(2), frac=P(3), st=None)
    _expect(lib, lib.d3d_cloud_keys, ok, ["xyz", "n"] + grid_order + ["keys", "frac", "st"],
            [(dict(xyz=None), b"null"), (dict(keys=None), b"null"), (dict(frac=None), b"null")] + bad_n("n") + grid_cases +
            [(dict(frac=ctypes.c_void_p((2 << 32) + 72)), b"alias"), (dict(keys=ctypes.c_void_p((1 << 32) + 119)), b"alias")])
    # heads
    need = lib.d3d_cloud_scratch_bytes(10)
    ok = dict(keys=P(1), n=10, s=P(2), sb=need, vox=P(3), nv=P(4), st=None)
    _expect(lib, lib.d3d_cloud_heads, ok, ["keys", "n", "s", "sb", "vox", "nv", "st"],
            [(dict(keys=None), b"null"), (dict(s=None), b"null"), (dict(vox=None), b"null"), (dict(nv=None), b"null")] + bad_n("n") +
            [(dict(sb=need - 1), b"scratch"), (dict(sb=0), b"scratch"), (dict(vox=ctypes.c_void_p((1 << 32) + 76)), b"alias"),
             (dict(nv=ctypes.c_void_p((2 << 32) + need - 1)), b"alias"), (dict(vox=ctypes.c_void_p((2 << 32) - 4)), b"alias")])
    # accumulate
    ok = dict(keys=P(1), order=P(2), vox=P(3), frac=P(4), nrm=P(5), col=P(6), n=10, nv=4, uk=P(7), cnt=P(8), acc=P(9), st=None)
    _expect(lib, lib.d3d_cloud_accumulate, ok, ["keys", "order", "vox", "frac", "nrm", "col", "n", "nv", "uk", "cnt", "acc", "st"],
            [(dict(keys=None), b"null"), (dict(order=None), b"null"), (dict(vox=None), b"null"), (dict(frac=None), b"null"),
             (dict(uk=None), b"null"), (dict(cnt=None), b"null"), (dict(acc=None), b"null")] + bad_n("n") +
            [(dict(nv=-1), b"n_voxels"), (dict(nv=11), b"n_voxels"), (dict(acc=ctypes.c_void_p((9 << 32) - 8), cnt=P(9)), b"alias"),
             (dict(acc=ctypes.c_void_p((5 << 32) + 116)), b"alias"), (dict(uk=P(2)), b"alias"),
             (dict(acc=ctypes.c_void_p((8 << 32) - 4 * 9 * 8 + 8)), b"alias")])
    # neighbours
    need = lib.d3d_cloud_scratch_bytes(4)
    ok = dict(uk=P(1), cnt=P(2), nv=4, nx=16, ny=8, nz=4, k=1, s=P(3), sb=need, keep=P(4), pos=P(5), nk=P(6), st=None)
    _expect(lib, lib.d3d_cloud_neighbours, ok, ["uk", "cnt", "nv", "nx", "ny", "nz", "k", "s", "sb", "keep", "pos", "nk", "st"],
            [(dict(uk=None), b"null"), (dict(cnt=None), b"null"), (dict(s=None), b"null"), (dict(keep=None), b"null"),
             (dict(pos=None), b"null"), (dict(nk=None), b"null")] + bad_n("nv") +
            [(dict(nx=0), b"grid"), (dict(ny=1 << 21), b"grid"), (dict(nz=-3), b"grid"), (dict(k=0), b"min_points"), (dict(k=-2), b"min_points"),
             (dict(sb=need - 1), b"scratch"), (dict(pos=P(4)), b"alias"), (dict(keep=ctypes.c_void_p((3 << 32) + 8)), b"alias"),
             (dict(nk=ctypes.c_void_p((5 << 32) + 12)), b"alias")])
    # finalize
    ok = dict(grid, uk=P(1), cnt=P(2), acc=P(3), keep=P(4), pos=P(5), nv=4, nk=3, xyz=P(6), nrm=P(7), col=P(8), out=P(9), st=None)
    _expect(lib, lib.d3d_cloud_finalize, ok, ["uk", "cnt", "acc", "keep", "pos", "nv", "nk"] + grid_order + ["xyz", "nrm", "col", "out", "st"],
            [(dict(uk=None), b"null"), (dict(cnt=None), b"null"), (dict(acc=None), b"null"), (dict(keep=None), b"null"),
             (dict(pos=None), b"null"), (dict(xyz=None), b"null"), (dict(out=None), b"null")] + bad_n("nv") +
            [(dict(nk=-1), b"n_kept"), (dict(nk=5), b"n_kept")] + grid_cases +
            [(dict(col=ctypes.c_void_p((7 << 32) + 35)), b"alias"), (dict(out=P(6)), b"alias"),
             (dict(xyz=ctypes.c_void_p((3 << 32) + 4 * 9 * 8 - 1)), b"alias")])
    # what is not an error: no points, no voxels, no optional arrays -- and nothing is launched for them
    assert lib.d3d_cloud_keys(None, 0, 0.0, 8.0, 0.0, 4.0, -1.0, 1.0, 0.5, None, None, None) == 0
    assert lib.d3d_cloud_accumulate(P(1), P(2), P(3), P(4), None, None, 10, 0, None, None, None, None) == 0
    assert lib.d3d_cloud_finalize(P(1), P(2), P(3), P(4), P(5), 4, 0, 0.0, 8.0, 0.0, 4.0, -1.0, 1.0, 0.5, None, None, None, None, None) == 0


def test_operator_refuses_cpu_tensors_bad_dtypes_and_shapes():
    g = unit_grid()
    xyz, nrm, col = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.merge_points(xyz, nrm, col, g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.merge_points(xyz, None, None, g, 3)
    for kw, msg in ((dict(xyz=xyz.double()), "xyz"), (dict(xyz=torch.zeros(5, 2)), "xyz"), (dict(xyz=torch.zeros(15)), "xyz"),
                    (dict(normal=torch.zeros(4, 3)), "normal"), (dict(normal=nrm.half()), "normal"), (dict(color=col.long()), "color"),
                    (dict(color=torch.zeros(5, 3, dtype=torch.uint8)), "color"), (dict(color=torch.zeros(5, 4, dtype=torch.int32)), "color"),
                    (dict(min_points=0), "min_points"), (dict(min_points=1.5), "min_points")):
        with pytest.raises(ValueError, match=msg):
            cloud.merge_points(**dict(dict(xyz=xyz, normal=nrm, color=col, grid=g), **kw))
    with pytest.raises(TypeError, match="CloudGrid"):
        cloud.merge_points(xyz, nrm, col, [0, 4, 0, 4, 0, 4])
    with pytest.raises(TypeError, match="Tensor"):
        cloud.merge_points(np.zeros((5, 3), np.float32), None, None, g)


def test_the_kernels_use_integer_atomic_add_only_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/cloud.hip").read())
    assert set(re.findall(r"\batomic\w*", hip)) == {"atomicAdd"}
    assert not re.search(r"unsafeAtomic|atomicAdd\s*\(\s*\(?\s*(float|double)\s*\*|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
    # every atomicAdd is a statement: its result is not used
    assert len(re.findall(r"(?:^|[;{}\)])\s*atomicAdd\(", hip, re.M)) == len(re.findall(r"\batomicAdd\(", hip)) == 2
    assert "fma" not in hip
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bcloud\.hip\b", make, re.M) and "-ffp-contract=off" in make
