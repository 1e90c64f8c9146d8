"""The cloud's outlier removal on the GPU (csrc/cloud_outliers.hip, cloud_outliers.point_distances / outlier_mask / filter_cloud):
D, nn, keep and the three sums bit-equal to the numpy restatements of tests/test_cloud_outliers.py -- on empty and unkeyed clouds,
on a cell of 5000 points, on single-point cells past one scan block, on cells that straddle waves and workgroups, on the
hand-computed cases, on a surface with floaters in any point order --; the filter on a merged cloud; the file tool; and the pipeline
stage on cloud_scene's block: the filtered PLY is the filter of the unfiltered one, and one rank and two write the same bytes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_outliers_scene as COS
import ortho_scene as OS
import test_cloud as TC
import test_cloud_outliers as TO
import texture_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _cuda(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _check(xyz, grid, settings, found=None):
    """The GPU's D, nn, sums, keep and info against the restatement, for every (k, alpha, min_neighbours) of settings; the
    restatement's search (k does not enter it) is made once."""
    from deep3d_aerial_amd import cloud_outliers as CO

    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    found = found or (TO.neighbours_numpy(xyz, grid) if len(xyz) <= 3000 else TO.neighbours_cells(xyz, grid))
    x = _cuda(xyz, np.float32)
    out = []
    for k, alpha, m in settings:
        want = TO.outliers_from(found, k, alpha, m)
        D, nn, sums = CO.point_distances(x, grid, k)
        assert D.is_cuda and D.dtype == torch.int32 and nn.dtype == torch.int32 and sums.dtype == torch.int64
        assert tuple(sums.tolist()) == want["sums"]
        assert np.array_equal(D.cpu().numpy(), want["D"]) and np.array_equal(nn.cpu().numpy(), want["nn"])
        keep, info = CO.outlier_mask(x, grid.border, grid.voxel, k, alpha, m)
        assert keep.is_cuda and keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want["keep"])
        assert info == want["info"], (info, want["info"])
        out.append(want)
    return out


def _in_voxels(vox, seed):
    """One point in each listed cell (a list of (ix, iy, iz), repeats allowed) of a unit grid, at a random place inside it."""
    rng = np.random.default_rng(seed)
    return (np.asarray(vox, np.float64) + rng.uniform(0.01, 0.99, (len(vox), 3))).astype(np.float32)


# ----------------------------------------------------------------------------------------
# sizes and runs
# ----------------------------------------------------------------------------------------
def test_no_point_one_point_two_points_and_only_unkeyed_points():
    g = TC.unit_grid()
    w = _check(np.zeros((0, 3), np.float32), g, [(8, 2.0, 0), (1, None, 1)])[0]
    assert w["D"].shape == (0,) and w["info"] == {"points": 0, "keyed": 0, "kept": 0, "mu": 0.0, "sigma": 0.0, "threshold": 0}
    w = _check(np.float32([[1.25, 2.5, 3.75]]), g, [(8, 2.0, 0), (32, 0.0, 1)])
    assert w[0]["D"].tolist() == [8192] and w[0]["keep"].tolist() == [True] and w[1]["keep"].tolist() == [False]
    w = _check(np.float32([[1.25, 2.5, 3.75], [1.25, 2.75, 3.75]]), g, [(1, 2.0, 0), (2, None, 1)])
    assert w[0]["D"].tolist() == [256, 256] and w[1]["D"].tolist() == [1280, 1280]
    gone = np.float32([[np.nan, 1, 1], [4, 1, 1], [1, -0.5, 1], [1, 1, np.inf], [9, 9, 9]])
    w = _check(gone, g, [(8, 2.0, 0), (1, None, 3)])[0]
    assert w["D"].tolist() == [-1] * 5 and w["info"]["keyed"] == 0 and not w["keep"].any()


def test_5000_points_in_one_cell():
    """Every point has 4999 candidates in its own cell, beside a few in the cells around it; k = 1, 8 and 32."""
    rng = np.random.default_rng(1)
    xyz = np.concatenate([_in_voxels([(2, 1, 3)] * 5000 + [(2, 1, 2), (1, 1, 3), (3, 2, 3), (0, 0, 0)], 2),
                          np.float32([[2.5, 1.5, 3.5]] * 3)])   # and three duplicates of the centre
    xyz = xyz[rng.permutation(len(xyz))]
    w = _check(xyz, TC.unit_grid(), [(1, 2.0, 0), (8, 1.0, 4000), (32, None, 2)], TO.neighbours_cells(xyz, TC.unit_grid()))
    assert w[0]["nn"].max() > 4000 and (w[0]["D"] == 0).sum() == 3 and 0 < w[1]["info"]["kept"] < 5000


@pytest.mark.parametrize("n", [4097, 2 * 4096 + 1])
def test_one_point_per_cell_past_one_and_two_scan_tiles(n):
    from deep3d_aerial_amd import cloud

    g = cloud.CloudGrid([0.0, 100.0, 0.0, 100.0, 0.0, 2.0], 1.0)
    k = np.arange(n)
    xyz = _in_voxels(np.stack([k % 100, k // 100 % 100, k // 10000], 1), n)
    xyz = xyz[np.random.default_rng(n).permutation(n)]
    w = _check(xyz, g, [(8, 2.0, 0), (3, 1.0, 2)])
    assert 0 < w[0]["info"]["kept"] <= n and 0 < w[1]["info"]["kept"] < n and w[0]["nn"].max() >= 4


def test_cells_that_straddle_waves_and_workgroups():
    from deep3d_aerial_amd import cloud

    lengths = [1, 2, 63, 64, 65, 255, 256, 257] * 3
    g = cloud.CloudGrid([0.0, 24.0, 0.0, 1.0, 0.0, 1.0], 1.0)   # the cells in a row: every cell's neighbours are the runs beside it
    vox = np.repeat(np.arange(len(lengths)), lengths)
    xyz = _in_voxels(np.stack([vox, 0 * vox, 0 * vox], 1), 8)
    settings = [(8, 2.0, 0), (32, 1.0, 70)]
    found = TO.neighbours_cells(xyz, g)
    w = _check(xyz, g, settings, found)                     # the points already in key order
    assert 0 < w[1]["info"]["kept"] < len(xyz)
    p = np.random.default_rng(10).permutation(len(xyz))
    _check(xyz[p], g, settings, tuple(a[p] for a in found))
    for skip in (1, 37):   # a shifted start: the cells meet the wave boundaries elsewhere
        _check(xyz[skip:], g, settings[:1], TO.neighbours_cells(xyz[skip:], g))


@pytest.mark.parametrize("case", TO.hand_cases(), ids=lambda c: c[0])
def test_the_hand_cases(case):
    _, xyz, g, k, alpha, m, D, nn, keep = case
    w = _check(xyz, g, [(k, alpha, m)])[0]
    assert w["D"].tolist() == D and w["nn"].tolist() == nn and w["keep"].tolist() == [bool(x) for x in keep]


def test_the_random_clouds_of_the_cpu_file():
    xyz, g = TO.random_cloud(4, 3000)
    _check(xyz, g, [(1, 1.0, 0), (8, 1.0, 3), (16, 2.0, 0), (17, 0.5, 1), (32, None, 5)])


# ----------------------------------------------------------------------------------------
# a surface with floaters
# ----------------------------------------------------------------------------------------
def surface(seed, n=20000, floaters=200):
    """n points on a jittered surface over 40 x 40 (about ten neighbours within the radius 0.5), floaters above and below it, and a
    few points outside the grid."""
    from deep3d_aerial_amd import cloud

    rng = np.random.default_rng(seed)
    g = cloud.CloudGrid([0.0, 40.0, -20.0, 20.0, 0.0, 6.0], 0.5)
    x, y = rng.uniform(0, 40, n), rng.uniform(-20, 20, n)
    z = 3.0 + np.sin(0.5 * x) * np.cos(0.4 * y) + rng.normal(0, 0.03, n)
    out = rng.uniform([0, -20, 0], [40, 20, 6], (floaters, 3))
    far = rng.uniform([-5, -25, -3], [45, 25, 9], (50, 3))
    xyz = np.concatenate([np.stack([x, y, z], 1), out, far]).astype(np.float32)
    is_floater = np.concatenate([np.zeros(n, bool), np.ones(floaters, bool), np.zeros(50, bool)])
    p = rng.permutation(len(xyz))
    return xyz[p], is_floater[p], g


def test_the_surface_is_bit_equal_under_three_shuffles_and_the_floaters_go():
    xyz, floater, g = surface(0)
    found = TO.neighbours_cells(xyz, g)
    settings = [(8, 2.0, 0), (8, None, 3)]
    w = _check(xyz, g, settings, found)
    for want in w:   # most floaters go, most of the surface stays
        assert (~want["keep"][floater]).mean() > 0.7 and want["keep"][~floater & found[0]].mean() > 0.9
    rng = np.random.default_rng(2)
    for _ in range(3):
        p = rng.permutation(len(xyz))
        _check(xyz[p], g, settings, tuple(a[p] for a in found))   # the per-point results, the shuffle undone


# ----------------------------------------------------------------------------------------
# the filter and the file tool
# ----------------------------------------------------------------------------------------
def _merged(seed):
    import test_cloud_gpu as TG
    from deep3d_aerial_amd import cloud

    xyz, nrm, col, g = TG.surface(seed, 3000)
    return xyz, nrm, col, g, cloud


@pytest.mark.parametrize("normals, colors", [(True, True), (True, False), (False, False)])
def test_filter_cloud_masks_every_array_of_a_merged_cloud(normals, colors):
    from deep3d_aerial_amd import cloud_outliers as CO

    xyz, nrm, col, g, cloud = _merged(3)
    c = cloud.merge_points(_cuda(xyz, np.float32), _cuda(nrm, np.float32) if normals else None, _cuda(col, np.int32) if colors else None, g)
    s = {"radius": 3 * g.voxel, "k": 6, "alpha": 1.0, "min_neighbours": 2}
    out, info = CO.filter_cloud(c, s, g.border)
    want = TO.outliers_from(TO.neighbours_numpy(c["xyz"].cpu().numpy(), cloud.CloudGrid(g.border, s["radius"])), 6, 1.0, 2)
    assert info == want["info"] and 0 < info["kept"] < info["points"] == len(want["keep"])
    assert sorted(out) == ["color", "count", "normal", "xyz"] and (out["normal"] is None) == (not normals) and (out["color"] is None) == (not colors)
    for name, t in c.items():
        if t is not None:
            assert out[name].is_cuda and out[name].dtype == t.dtype and out[name].is_contiguous()
            assert np.array_equal(out[name].cpu().numpy(), t.cpu().numpy()[want["keep"]], equal_nan=True), name
    # the border may ride in the settings
    out2, info2 = CO.filter_cloud(c, dict(s, border=g.border))
    assert info2 == info and torch.equal(out2["xyz"], out["xyz"])


def test_the_file_tool_writes_the_masked_cloud_byte_for_byte(tmp_path):
    xyz, nrm, col, g, cloud = _merged(4)
    src = tmp_path / "in.ply"
    settings = {"path": str(src), "border": g.border, "voxel": g.voxel, "min_points": 1}
    cloud.build_and_write(_cuda(xyz, np.float32), _cuda(nrm, np.float32), _cuda(col, np.int32), settings)
    c = cloud.read_cloud_ply(str(src))
    out = tmp_path / "cli" / "out.ply"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.cloud_outliers", "--cloud", str(src), "--out", str(out),
           "--border=%s" % ",".join(repr(b) for b in g.border), "--radius=%r" % (3 * g.voxel), "--k=6", "--alpha=1", "--min_neighbours=2"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    keep = TO.outliers_from(TO.neighbours_numpy(c["xyz"], cloud.CloudGrid(g.border, 3 * g.voxel)), 6, 1.0, 2)["keep"]
    assert 0 < keep.sum() < len(keep) and "kept %d of %d points" % (keep.sum(), len(keep)) in r.stdout
    assert out.read_bytes() == cloud.cloud_ply_bytes(c["xyz"][keep], c["normal"][keep], c["color"][keep], c["count"][keep])


# ----------------------------------------------------------------------------------------
# the pipeline stage
# ----------------------------------------------------------------------------------------
def _launch(n_ranks, out_dir, border, voxel, min_points, o):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "cloud_outliers_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel), str(min_points), repr(o["radius"]), str(o["k"]), "none" if o["alpha"] is None else repr(o["alpha"]),
           str(o["min_neighbours"])]
    res = subprocess.run(["timeout", "-k", "10", "300"] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def _files(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(folder) for f in fs)


def test_the_pipeline_filters_the_cloud_it_writes_and_two_ranks_write_the_same_bytes(tmp_path):
    from deep3d_aerial_amd import cloud, cloud_outliers as CO

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    o = {"radius": 3 * voxel, "k": 8, "alpha": 1.0, "min_neighbours": 4}
    off, on, two = tmp_path / "off", tmp_path / "on", tmp_path / "two"
    tm0, tm1 = {}, {}
    COS.run(str(off), border, voxel, 1, None, timings=tm0)
    COS.run(str(on), border, voxel, 1, o, timings=tm1)
    assert "cloud_outliers" not in tm0 and tm0["cloud_s"] > 0
    # the filtered file is the filter of the unfiltered file
    first = cloud.read_cloud_ply(str(off / "cloud.ply"))
    dev = {name: (None if v is None else torch.from_numpy(v).cuda()) for name, v in first.items()}
    want, info = CO.filter_cloud(dev, o, border)
    assert 0 < info["kept"] < info["points"] == len(first["count"]) and info["points"] > 300
    assert tm1["cloud_outliers"] == info
    data = (on / "cloud.ply").read_bytes()
    assert data == cloud.cloud_ply_bytes(want["xyz"], want["normal"], want["color"], want["count"])
    # and of the restatement's mask
    keep = TO.outliers_from(TO.neighbours_numpy(first["xyz"], cloud.CloudGrid(border, o["radius"])), 8, 1.0, 4)["keep"]
    assert np.array_equal(want["xyz"].cpu().numpy(), first["xyz"][keep])
    # the key adds no product and removes none
    assert _files(str(off)) == _files(str(on)) and "cloud.ply" in _files(str(off))
    # two ranks
    out2 = _launch(2, two, border, voxel, 1, o)
    assert "rank 0/2" in out2 and "rank 1/2" in out2 and "'kept': %d" % info["kept"] in out2
    assert (two / "cloud.ply").read_bytes() == data
