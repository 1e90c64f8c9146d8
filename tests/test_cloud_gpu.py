"""The merged point cloud on the GPU (csrc/cloud.hip cloud_*, cloud.merge_points): bit-equal to the numpy restatement of
tests/test_cloud.py in every output array -- on empty and dropped clouds, on runs of equal keys that straddle waves, workgroups
and scan tiles, on sums past 2^32, on the crafted border, key-packing and filter cases --, the same bytes for any point order; the
file; and the pipeline stage on ortho_scene's block: one rank and two write the same PLY, whose colours are the byte means of the
members' pixels."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_scene as CS
import ortho_scene as OS
import test_cloud as TC
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _cuda(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _host(c):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in c.items()}


def _gpu(xyz, nrm, col, grid, k=1):
    from deep3d_aerial_amd import cloud

    c = cloud.merge_points(_cuda(xyz, np.float32).reshape(-1, 3), None if nrm is None else _cuda(nrm, np.float32).reshape(-1, 3),
                           None if col is None else _cuda(col, np.int32).reshape(-1, 3), grid, k)
    assert all(v is None or v.is_cuda for v in c.values()) and sorted(c) == ["color", "count", "normal", "xyz"]
    return _host(c)


def _check(xyz, nrm, col, grid, k=1):
    want = TC.cloud_numpy(xyz, nrm, col, grid, k)
    TC.same_cloud(_gpu(xyz, nrm, col, grid, k), want)
    return want


def _attrs(n, seed):
    """Random normals (a few NaN, Inf and huge ones among them) and colours (a few outside 0 .. 255)."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-6).astype(np.float32)
    bad = rng.uniform(size=n) < 0.02
    nrm[bad, rng.integers(0, 3, bad.sum())] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 5e3, -1e30]), bad.sum())
    col = rng.integers(0, 256, (n, 3)).astype(np.int32)
    odd = rng.uniform(size=n) < 0.02
    col[odd, rng.integers(0, 3, odd.sum())] = rng.choice(np.int32([-7, 256, 1000, -(1 << 31), (1 << 31) - 1]), odd.sum())
    return nrm, col


def _in_voxels(vox, seed):
    """One point in each listed voxel (a list of (ix, iy, iz), repeats allowed) of a unit grid, at a random place inside it."""
    rng = np.random.default_rng(seed)
    return (np.asarray(vox, np.float64) + rng.uniform(0.01, 0.99, (len(vox), 3))).astype(np.float32)


# ----------------------------------------------------------------------------------------
# sizes and runs
# ----------------------------------------------------------------------------------------
def test_no_point_one_point_and_only_dropped_points():
    g = TC.unit_grid()
    empty = np.zeros((0, 3), np.float32)
    for nrm, col in ((None, None), (empty, np.zeros((0, 3), np.int32))):
        c = _gpu(empty, nrm, col, g)
        assert c["xyz"].shape == (0, 3) and c["count"].shape == (0,) and (c["normal"] is None) == (nrm is None)
    one = np.float32([[1.25, 2.5, 3.75]])
    w = _check(one, np.float32([[0, 3, 4]]), np.int32([[1, 2, 3]]), g)
    assert w["count"].tolist() == [1] and w["color"].tolist() == [[1, 2, 3]]
    gone = np.float32([[np.nan, 1, 1], [4, 1, 1], [1, -0.5, 1], [1, 1, np.inf], [9, 9, 9]])
    for k in (1, 3):
        w = _check(gone, np.ones((5, 3), np.float32), np.zeros((5, 3), np.int32), g, k)
        assert w["count"].shape == (0,)
    # dropped points among kept ones, without the optional arrays
    w = _check(np.concatenate([gone, one, gone, one]), None, None, g)
    assert w["count"].tolist() == [2]


@pytest.mark.parametrize("normals, colors", [(True, True), (True, False), (False, True), (False, False)])
def test_5000_points_in_one_voxel(normals, colors):
    """A run longer than a workgroup and longer than GEOM_SCAN_TILE, beside a few neighbours."""
    rng = np.random.default_rng(1)
    xyz = _in_voxels([(2, 1, 3)] * 5000 + [(2, 1, 2), (0, 0, 0), (3, 3, 3)], 2)
    xyz = xyz[rng.permutation(len(xyz))]
    nrm, col = _attrs(len(xyz), 3)
    w = _check(xyz, nrm if normals else None, col if colors else None, TC.unit_grid())
    assert sorted(w["count"].tolist()) == [1, 1, 1, 5000]


def test_70000_points_with_r_near_65535_pass_two_to_the_32():
    """S = 70 000 x 65535 > 2^32 in every axis: a 32-bit accumulator would wrap."""
    top = np.float32(2.0 - 2.0 ** -20)
    assert float(top) == 2.0 - 2.0 ** -20
    xyz = np.full((70000, 3), top, np.float32)
    nrm = np.tile(np.float32([[0.0, 0.6, 0.8]]), (70000, 1))
    col = np.tile(np.int32([[255, 254, 0]]), (70000, 1))
    w = _check(xyz, nrm, col, TC.unit_grid())
    assert w["count"].tolist() == [70000] and w["color"].tolist() == [[255, 254, 0]] and 70000 * 65535 > 1 << 32
    assert w["xyz"][0, 0] == np.float32(1.0 + (70000 * 65535 + 35000.0) / (65536.0 * 70000))


@pytest.mark.parametrize("n", [4097, 2 * 4096 + 1])
def test_one_point_per_voxel_past_one_and_two_scan_tiles(n):
    from deep3d_aerial_amd import cloud

    g = cloud.CloudGrid([0.0, 100.0, 0.0, 100.0, 0.0, 2.0], 1.0)
    k = np.arange(n)
    xyz = _in_voxels(np.stack([k % 100, k // 100 % 100, k // 10000], 1), n)
    xyz = xyz[np.random.default_rng(n).permutation(n)]
    nrm, col = _attrs(n, n + 1)
    w = _check(xyz, nrm, col, g)
    assert (w["count"] == 1).all() and len(w["count"]) == n
    w = _check(xyz, None, col, g, 9)     # one layer, one point per voxel: the voxels with all eight neighbours in the layer pass
    assert 0 < len(w["count"]) < n


def test_runs_that_straddle_waves_and_workgroups():
    from deep3d_aerial_amd import cloud

    lengths = [1, 2, 63, 64, 65, 255, 256, 257] * 12
    g = cloud.CloudGrid([0.0, 10.0, 0.0, 10.0, 0.0, 1.0], 1.0)
    vox = np.repeat(np.arange(len(lengths)), lengths)
    xyz = _in_voxels(np.stack([vox % 10, vox // 10, 0 * vox], 1), 8)
    nrm, col = _attrs(len(xyz), 9)
    rng = np.random.default_rng(10)
    w = _check(xyz, nrm, col, g)                      # the points already in key order
    assert w["count"].tolist() == lengths
    p = rng.permutation(len(xyz))
    TC.same_cloud(_gpu(xyz[p], nrm[p], col[p], g), w)
    # a shifted start: the runs meet the wave boundaries elsewhere
    for skip in (1, 37):
        _check(xyz[skip:], nrm[skip:], col[skip:], g)


# ----------------------------------------------------------------------------------------
# the crafted cases of the CPU file
# ----------------------------------------------------------------------------------------
def test_the_crafted_border_tie_and_key_packing_cases():
    for case in (TC.tie_case, TC.faces_case, TC.packing_case):
        xyz, nrm, col, g = case()
        _check(xyz, nrm, col, g)
    g = TC.unit_grid()
    a = _gpu(np.float32([[-0.0, -0.0, -0.0], [0.25, 0.5, -0.0]]), None, None, g)
    b = _gpu(np.float32([[0.0, 0.0, 0.0], [0.25, 0.5, 0.0]]), None, None, g)
    TC.same_cloud(a, b)
    xyz = np.float32([[0.5, 0.5, 0.5]] * 2 + [[1.5, 0.5, 0.5]] * 2 + [[2.5, 0.5, 0.5]] * 2 + [[3.5, 0.5, 0.5]])
    nrm = np.float32([[np.nan, 0, 1], [0, 0, 1], [0.6, 0, 0.8], [-0.6, 0, -0.8], [np.inf, 0, 0], [0, 2e3, 0], [3, 0, 4]])
    w = _check(xyz, nrm, None, g)
    assert w["normal"][:3].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]]
    from deep3d_aerial_amd import cloud

    g2 = cloud.CloudGrid([0.0, 3.5, 0.0, 1.0, 0.0, 1.0], 1.0)
    assert _check(np.float32([[3.5, 0.5, 0.5], [3.99, 0.5, 0.5], [4.0, 0.5, 0.5]]), None, None, g2)["count"].tolist() == [2]


def test_the_crafted_filter_cases():
    from deep3d_aerial_amd import cloud

    xyz, _, _, g = TC.filter_case()
    sizes = [len(_check(xyz, None, None, g, k)["count"]) for k in (1, 2, 3, 5, 6)]
    assert sizes == [6, 4, 1, 1, 0]
    g1 = cloud.CloudGrid([0.0, 5.0, 0.0, 1.0, 0.0, 1.0], 1.0)
    assert _check(np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]]), None, None, g1, 3)["count"].tolist() == [1]
    gb = TC.big_grid()
    v = gb.voxel
    c0, c1 = np.float32((TC.M + 0.5) * v), np.float32((TC.M - 0.5) * v)
    pts = np.float32([[c0, c0, c0], [c1, c0, c0], [np.float32(0.5 * v), c0, c0]])
    assert len(_check(pts, None, None, gb, 2)["count"]) == 2


# ----------------------------------------------------------------------------------------
# a surface with duplicates and outliers
# ----------------------------------------------------------------------------------------
def surface(seed, n=2500):
    """n points on a jittered surface over a 12 x 11 x 5 grid of 0.5 (about 8 per occupied voxel), 150 scattered outliers and 100
    points outside the grid."""
    from deep3d_aerial_amd import cloud

    rng = np.random.default_rng(seed)
    g = cloud.CloudGrid([10.0, 16.0, -3.0, 2.5, 0.0, 2.5], 0.5)
    x, y = rng.uniform(10, 16, n), rng.uniform(-3, 2.5, n)
    z = 1.2 + 0.5 * np.sin(x) * np.cos(y) + rng.normal(0, 0.05, n)
    out = rng.uniform([10, -3, 0], [16, 2.5, 2.5], (150, 3))
    far = rng.uniform([5, -8, -3], [21, 7, 6], (100, 3))
    xyz = np.concatenate([np.stack([x, y, z], 1), out, far]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    nrm, col = _attrs(len(xyz), seed + 1)
    return xyz, nrm, col, g


def test_the_surface_is_bit_equal_for_any_point_order_and_the_filter_drops_what_the_restatement_drops():
    xyz, nrm, col, g = surface(0)
    w1 = _check(xyz, nrm, col, g, 1)
    assert 4 < w1["count"].mean() < 15
    rng = np.random.default_rng(2)
    for _ in range(2):
        p = rng.permutation(len(xyz))
        TC.same_cloud(_gpu(xyz[p], nrm[p], col[p], g, 1), w1)
    # the points split in two batches and swapped: the multiset is the same
    h = len(xyz) // 3
    TC.same_cloud(_gpu(np.concatenate([xyz[h:], xyz[:h]]), np.concatenate([nrm[h:], nrm[:h]]), np.concatenate([col[h:], col[:h]]), g), w1)
    for k in (4, 40):
        w = _check(xyz, nrm, col, g, k)
        got = _gpu(xyz, nrm, col, g, k)
        dropped = int((~w["kept"]).sum())
        assert 0 < dropped < len(w["kept"]) and len(got["count"]) == len(w["kept"]) - dropped
        # the kept voxels are the unfiltered voxels with the same outputs: the filter only selects
        for name in ("xyz", "normal", "color", "count"):
            assert np.array_equal(got[name], w1[name][w["kept"]], equal_nan=True)


def test_build_and_write_writes_what_merge_points_returns(tmp_path):
    from deep3d_aerial_amd import cloud

    xyz, nrm, col, g = surface(3, 3000)
    path = tmp_path / "out" / "c.ply"
    settings = {"path": str(path), "border": g.border, "voxel": g.voxel, "min_points": 2}
    for n_, c_ in ((nrm, col), (nrm, None), (None, None)):
        c, s = cloud.build_and_write(_cuda(xyz, np.float32), _cuda(n_, np.float32), _cuda(c_, np.int32), settings)
        back = cloud.read_cloud_ply(str(path))
        TC.same_cloud(back, _host(c))
        TC.same_cloud(back, TC.cloud_numpy(xyz, n_, c_, g, 2))
        assert s["points"] == len(xyz) and s["voxels"] == len(back["count"]) and abs(s["mean_count"] - back["count"].mean()) < 1e-9


# ----------------------------------------------------------------------------------------
# the pipeline stage
# ----------------------------------------------------------------------------------------
def _launch(n_ranks, out_dir, border, voxel, min_points):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "cloud_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel), str(min_points)]
    res = subprocess.run(["timeout", "-k", "10", "300"] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def _pixel_colors(result, image):
    """The colour of every point of a result from the reference image: its pixel is the one whose fused position it carries."""
    fm = result["final_mask"].cpu().numpy()
    avg = np.ascontiguousarray(result["avg_xyz_world"].cpu().numpy().transpose(1, 2, 0))
    ys, xs = np.nonzero(fm)
    at = {avg[y, x].tobytes(): (y, x) for y, x in zip(ys, xs)}
    assert len(at) == len(ys)   # no two confirmed pixels share a position
    pix = [at[p.tobytes()] for p in result["points"]["xyz"].cpu().numpy()]
    return image[[p[0] for p in pix], [p[1] for p in pix]].astype(np.int32).reshape(-1, 3)


def test_one_rank_and_two_ranks_write_the_same_coloured_cloud(tmp_path):
    from deep3d_aerial_amd import cloud

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    K = 3
    one, two, plain = tmp_path / "one", tmp_path / "two", tmp_path / "plain"
    tm = {}
    res = CS.run(str(one), border, voxel, K, timings=tm)
    assert tm["cloud_s"] > 0 and (one / "cloud.ply").exists()
    out2 = _launch(2, two, border, voxel, K)
    assert "rank 0/2" in out2 and "rank 1/2" in out2
    data = (one / "cloud.ply").read_bytes()
    assert data == (two / "cloud.ply").read_bytes()
    # the colours of the fused points are their pixels' bytes, and the cloud is the restatement's merge of them
    images = {"scene_%02d" % i: v["image"] for i, v in enumerate(scene.views)}
    names = {r["name"] for r in scene.view_records()}
    assert {r["ref"] for r in res} <= names and set(images) == names
    xyz = np.concatenate([r["points"]["xyz"].cpu().numpy() for r in res])
    nrm = np.concatenate([r["points"]["normal"].cpu().numpy() for r in res])
    col = np.concatenate([r["points"]["color"].cpu().numpy() for r in res])
    pix = np.concatenate([_pixel_colors(r, images[r["ref"]]) for r in res])
    assert len(xyz) > 1000 and col.dtype == np.int32 and np.array_equal(col, pix)
    want = TC.cloud_numpy(xyz, nrm, pix, cloud.CloudGrid(border, voxel), K)
    back = cloud.read_cloud_ply(str(one / "cloud.ply"))
    TC.same_cloud(back, want)
    assert len(back["count"]) > 300 and back["count"].max() > 1 and len(back["count"]) == int(want["kept"].sum())
    assert len(np.unique(back["color"], axis=0)) > 50
    # without the key: no file, no colour, the same points
    tm0 = {}
    res0 = CS.run(str(plain), border, voxel, K, cloud=False, timings=tm0)
    assert "cloud_s" not in tm0 and not (plain / "cloud.ply").exists() and all(r["points"]["color"] is None for r in res0)
    assert sorted(os.listdir(plain)) == sorted(f for f in os.listdir(one) if f != "cloud.ply")
    assert np.array_equal(np.concatenate([r["points"]["xyz"].cpu().numpy() for r in res0]), xyz)


def test_the_command_line_merges_the_fused_arrays(tmp_path):
    from deep3d_aerial_amd import cloud, pipeline

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    res = CS.run(str(tmp_path / "run"), border, voxel, 1, cloud=False)
    pipeline.save_fused(res, str(tmp_path / "fused"))
    out = tmp_path / "cli" / "c.ply"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.cloud", "--fused", str(tmp_path / "fused"), "--out", str(out),
           "--border=%s" % ",".join(repr(b) for b in border), "--voxel=%r" % voxel, "--min_points=2"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "points per voxel" in r.stdout
    xyz, nrm = cloud.read_fused(str(tmp_path / "fused"))
    back = cloud.read_cloud_ply(str(out))
    assert back["color"] is None and back["normal"] is not None
    TC.same_cloud(back, TC.cloud_numpy(xyz, nrm, None, cloud.CloudGrid(border, voxel), 2))
