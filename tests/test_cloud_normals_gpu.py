"""The normals of a point cloud on the GPU (csrc/cloud_normals.hip, cloud_normals.estimate) against the numpy restatement of
tests/cloud_normals_scene.py: the ten sums bit for bit, the count exactly, the flatness within one, the normal within 1e-6 rad of
numpy.linalg.eigh's wherever the two smallest eigenvalues are apart -- at no point, one, two, three collinear ones, two tiles, and
on the scene with its duplicates, corner cells, a pair exactly one radius apart and unkeyed points; the same bits under a
permutation; both orientations; and the file tool."""
import numpy as np
import pytest
import torch

import cloud_normals_scene as NS
from deep3d_aerial_amd import cloud

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a, np.float32).reshape(-1, 3)).cuda()   # (a copy: the scene's arrays are read-only)


def _estimate(xyz, border, radius, z_down=False):
    from deep3d_aerial_amd import cloud_normals as CN

    n = len(xyz)
    normals, count, flatness, sums = CN.estimate(_cuda(xyz), border, radius, z_down, return_sums=True)
    assert all(t.is_cuda for t in (normals, count, flatness, sums))
    assert (normals.dtype, count.dtype, flatness.dtype, sums.dtype) == (torch.float32, torch.int32, torch.int32, torch.int64)
    assert (tuple(normals.shape), tuple(count.shape), tuple(flatness.shape), tuple(sums.shape)) == ((n, 3), (n,), (n,), (n, 10))
    three = CN.estimate(_cuda(xyz), border, radius, z_down)
    assert len(three) == 3 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(three, (normals, count, flatness)))
    return normals.cpu().numpy(), count.cpu().numpy(), flatness.cpu().numpy(), sums.cpu().numpy()


def _check(got, want, z_down=False):
    """got of _estimate against want = (sums, normal, count, flatness, well) of the restatement."""
    normals, count, flatness, sums = got
    w_sums, w_normal, w_count, w_flat, well = want
    assert np.array_equal(sums, w_sums)
    assert np.array_equal(count, w_count)
    has = w_normal.any(1)
    assert np.array_equal(normals.any(1), has)                                    # the degenerate points are the same ones
    assert not normals[~has].any() and (flatness[~has] == -1).all()
    assert (np.abs(flatness[has].astype(np.int64) - w_flat[has]) <= 1).all()
    n64 = normals.astype(np.float64)
    assert np.abs((n64[has] ** 2).sum(1) - 1.0).max() < 1e-6 if has.any() else True
    up = n64[has, 2] * (-1.0 if z_down else 1.0)
    assert (up >= 0).all()
    if well.any():
        off = NS.angle(n64[well], w_normal[well])
        print("largest angle to eigh's normal %.3g rad over %d points" % (off.max(), well.sum()))
        assert off.max() < 1e-6
        assert ((n64[well] * w_normal[well]).sum(1) > 0).all()                    # and the same side


@pytest.mark.parametrize("n", [0, 1, 2])
def test_no_point_one_point_and_two_points(n):
    g = cloud.CloudGrid([0, 8, 0, 8, 0, 8], 2.0)
    xyz = np.float32([[3, 3, 1], [4, 3.5, 1.25]])[:n]
    s = NS.sums_numpy(xyz, g)
    got = _estimate(xyz, g.border, g.voxel)
    _check(got, (s,) + NS.normals_numpy(s))
    assert got[1].tolist() == [n] * n and not got[0].any() and (got[2] == -1).all()


def test_three_collinear_points_a_wall_and_a_plane():
    g = cloud.CloudGrid([0, 8, 0, 8, 0, 8], 2.0)
    line = np.float32([[1, 1, 1], [1.5, 1.5, 1.5], [2, 2, 2]])
    got = _estimate(line, g.border, g.voxel)
    s = NS.sums_numpy(line, g)
    _check(got, (s,) + NS.normals_numpy(s))
    assert got[1].tolist() == [3, 3, 3] and not got[0].any() and got[2].tolist() == [-1, -1, -1]
    for z_down in (False, True):
        wall = np.float32([[3, 3, 3], [3, 4, 3], [3, 3, 4], [3, 4, 4]])           # n . up == 0: the first non-zero component positive
        got = _estimate(wall, g.border, g.voxel, z_down)
        assert np.array_equal(got[0], np.float32([[1, 0, 0]] * 4)) and got[2].tolist() == [0] * 4
        plane = np.float32([[3, 3, 1], [4, 3, 1], [3, 4, 1], [2, 3, 1], [3, 2.5, 1], [3, 3, 5.5], [9, 3, 1]])
        got = _estimate(plane, g.border, g.voxel, z_down)
        assert np.array_equal(got[0][:5], np.float32([[0, 0, -1 if z_down else 1]] * 5)) and got[1].tolist() == [5, 4, 5, 4, 5, 1, 0]
        s = NS.sums_numpy(plane, g)
        _check(got, (s,) + NS.normals_numpy(s, z_down), z_down)


def test_257_points_two_tiles():
    xyz = NS.scene()[0][:257]
    g = cloud.CloudGrid(NS.BORDER, 5.0)            # the first points of the scene are sparse: a wider radius finds neighbours
    s = NS.sums_numpy(xyz, g)
    want = (s,) + NS.normals_numpy(s)
    assert want[1].any(1).sum() > 200
    _check(_estimate(xyz, g.border, g.voxel), want)


@pytest.mark.parametrize("z_down", [False, True], ids=["z_up", "z_down"])
def test_the_scene_and_a_permutation_of_it(z_down):
    xyz, parts = NS.scene()
    got = _estimate(xyz, NS.BORDER, NS.RADIUS, z_down)
    _check(got, NS.expected(z_down), z_down)
    assert (got[1][parts["unkeyed"]] == 0).all() and got[1][parts["apart"]].tolist() == [1, 1]
    if z_down:                                                                   # the other orientation is the negation, bit for bit
        up = _estimate(xyz, NS.BORDER, NS.RADIUS, False)
        flip = got[0][:, 2] != 0
        assert flip.sum() > 700 and np.array_equal(got[0][flip], -up[0][flip]) and np.array_equal(got[0][~flip], up[0][~flip])
        assert np.array_equal(got[2], up[2]) and np.array_equal(got[3], up[3])
    p = np.random.default_rng(11).permutation(len(xyz))
    again = _estimate(xyz[p], NS.BORDER, NS.RADIUS, z_down)
    for a, b in zip(got, again):
        assert np.array_equal(a[p].view(np.uint8), b.view(np.uint8))             # per point: the same bits in another order


def test_the_file_tool_adds_normals_and_keeps_the_colour(tmp_path, capsys):
    from deep3d_aerial_amd import cloud_compare as CC, cloud_normals as CN

    xyz, _ = NS.scene()
    xyz = xyz[:750]                                                              # (a NaN does not survive a comparison of files)
    col = np.random.default_rng(1).integers(0, 256, (len(xyz), 3)).astype(np.uint8)
    src, out = tmp_path / "in.ply", tmp_path / "out" / "n.ply"
    src.write_bytes(CN.normals_ply_bytes(xyz, np.zeros_like(xyz), col))
    args = ["--cloud", str(src), "--out", str(out), "--border=%s" % ",".join(repr(v) for v in NS.BORDER), "--radius=%r" % NS.RADIUS]
    assert CN.main(args + ["--min_count=10"]) == str(out)
    assert "750 points" in capsys.readouterr().out
    normals, count, _ = CN.estimate(_cuda(xyz), NS.BORDER, NS.RADIUS)
    normals, count = normals.cpu().numpy(), count.cpu().numpy()
    got_xyz, got_n = CC.read_xyz_ply(out, normals=True)
    assert np.array_equal(got_xyz, xyz) and np.array_equal(CC.vertex_columns(CC.read_vertex_ply(out), ("red", "green", "blue"), np.uint8), col)
    few = count < 10
    assert 0 < few.sum() < 100 and not got_n[few].any() and np.array_equal(got_n[~few], normals[~few])
    CN.main(args + ["--z_down"])
    down = CC.read_xyz_ply(out, normals=True)[1]
    assert np.array_equal(down, -normals) or np.array_equal(down[normals[:, 2] != 0], -normals[normals[:, 2] != 0])
