"""The normals of a point cloud without a GPU (deep3d_aerial_amd/cloud_normals.py, csrc/cloud_normals.hip): the restated rule by
hand, the scene the GPU tests use, the header, the binding and the library, the entry point's and the operator's refusals, the PLY
reader's normals and the command line."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import cloud_normals_scene as NS
import test_cloud as TC
from deep3d_aerial_amd import _lib, cloud, cloud_compare as CC, cloud_normals as CN

NEW_SYMBOLS = ("d3d_cloud_normals_scratch_bytes", "d3d_cloud_normals")


# ----------------------------------------------------------------------------------------
# the rule by hand
# ----------------------------------------------------------------------------------------
def test_the_rule_by_hand():
    g = cloud.CloudGrid([0, 8, 0, 8, 0, 8], 2.0)
    # five points of the plane z = 1 within a radius of the first, one two radii above (nobody's neighbour), one outside
    xyz = np.float32([[3, 3, 1], [4, 3, 1], [3, 4, 1], [2, 3, 1], [3, 2.5, 1], [3, 3, 5.5], [9, 3, 1]])
    s = NS.sums_numpy(xyz, g)
    assert s[0].tolist() == [5, 0, 256, 512 - 512, 2 * 512 * 512, 0, 0, 512 * 512 + 256 * 256, 0, 0]
    assert s[5].tolist() == [1] + [0] * 9 and s[6].tolist() == [0] * 10
    n, k, f, well = NS.normals_numpy(s)
    assert np.array_equal(n[0], [0, 0, 1]) and k[0] == 5 and f[0] == 0 and well[0]
    assert np.array_equal(NS.normals_numpy(s, z_down=True)[0][0], [0, 0, -1])
    assert not n[5].any() and f[5] == -1 and k[5] == 1 and not n[6].any() and f[6] == -1 and k[6] == 0
    # strictly inside the radius: a point exactly one radius away is no neighbour, one a float below it is
    for dx, want in ((2.0, 1), (float(np.nextafter(np.float32(2), np.float32(0))), 2)):
        assert NS.sums_numpy(np.float32([[0, 3, 3], [dx, 3, 3]]), g)[0, 0] == want
    # three collinear points: no plane.  A vertical wall x = 3: n . up == 0, the first non-zero component is made positive
    line = np.float32([[1, 1, 1], [1.5, 1.5, 1.5], [2, 2, 2]])
    n, k, f, _ = NS.normals_numpy(NS.sums_numpy(line, g))
    assert not n.any() and k.tolist() == [3, 3, 3] and f.tolist() == [-1] * 3
    wall = np.float32([[3, 3, 3], [3, 4, 3], [3, 3, 4], [3, 4, 4]])
    for z_down in (False, True):
        assert np.array_equal(NS.normals_numpy(NS.sums_numpy(wall, g), z_down)[0], [[1, 0, 0]] * 4)


def test_the_scene_is_what_the_gpu_tests_need():
    xyz, parts = NS.scene()
    g = NS.grid()
    s, n, k, f, well = NS.expected()
    assert len(xyz) == 753 and g.n == (11, 11, 6)
    keyed = TC.keys_numpy(xyz, g) != np.iinfo(np.int64).max
    assert keyed[:750].all() and not keyed[parts["unkeyed"]].any() and not k[parts["unkeyed"]].any()
    assert (k[parts["duplicates"]] >= 40 + 3).all() and k[parts["apart"]].tolist() == [1, 1] and (k[parts["corners"]] == 4).all()
    cells = TC.cells_numpy(xyz, g)[1][parts["corners"]]
    assert (cells[:4] == 0).all() and (cells[4:] == np.array(g.n) - 1).all()
    d = xyz[parts["apart"]].astype(np.float64)
    assert ((d[0] - d[1]) ** 2).sum() == NS.RADIUS ** 2
    # at most 5 % of the points with a normal have their two smallest eigenvalues too close for eigh's vector to be defined
    has = n.any(1)
    assert has.sum() >= 740 and (~well[has]).mean() <= 0.05
    assert (n[has, 2] >= 0).all() and np.allclose((n[has] ** 2).sum(1), 1.0, atol=1e-12)
    # the fitted normals are the surface's: within 0.3 rad of the analytic normal away from the blocks' walls, where the surface bends little
    x, y = xyz[:700, 0].astype(np.float64), xyz[:700, 1].astype(np.float64)
    e = 1e-4
    gx = (NS.CRS.height(x + e, y) - NS.CRS.height(x - e, y)) / (2 * e)
    gy = (NS.CRS.height(x, y + e) - NS.CRS.height(x, y - e)) / (2 * e)
    flat = f[:700] <= 2
    off = NS.angle(n[:700], np.stack([-gx, -gy, np.ones(700)], 1))
    assert flat.sum() > 50 and off[flat].max() < 0.3 and np.median(off) < 0.15


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
    assert lib.d3d_cloud_normals_scratch_bytes.restype is ctypes.c_size_t
    assert lib.d3d_cloud_normals_scratch_bytes(0) > 0 and lib.d3d_cloud_normals_scratch_bytes(1_000_000) >= 16 * 1_000_000
    for bad in (-1, 1 << 31):
        assert lib.d3d_cloud_normals_scratch_bytes(bad) == 0, bad


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    need = lib.d3d_cloud_normals_scratch_bytes(10)
    ok = dict(xyz=P(1), keys=P(2), order=P(3), n=10, nx=16, ny=8, nz=4, h=0.5, zd=0, s=P(4), sb=need, nrm=P(5), cnt=P(6), flat=P(7), sums=P(8),
              st=None)
    order = ["xyz", "keys", "order", "n", "nx", "ny", "nz", "h", "zd", "s", "sb", "nrm", "cnt", "flat", "sums", "st"]
    TC._expect(lib, lib.d3d_cloud_normals, ok, order,
               [(dict([(name, None)]), b"null") for name in ("xyz", "keys", "order", "s", "nrm", "cnt", "flat")] +
               [(dict(n=-1), b"n_points"), (dict(n=1 << 31), b"n_points"), (dict(nx=0), b"grid"), (dict(ny=1 << 21), b"grid"), (dict(nz=-3), b"grid"),
                (dict(h=0.0), b"cap"), (dict(h=-1.0), b"cap"), (dict(h=math.nan), b"cap"), (dict(h=math.inf), b"cap"),
                (dict(zd=2), b"z_down"), (dict(zd=-1), b"z_down"), (dict(sb=need - 1), b"scratch"), (dict(sb=0), b"scratch"),
                (dict(cnt=P(7)), b"alias"), (dict(nrm=ctypes.c_void_p((1 << 32) + 119)), b"alias"),
                (dict(sums=ctypes.c_void_p((4 << 32) + need - 1)), b"alias"), (dict(sums=ctypes.c_void_p((5 << 32) + 119)), b"alias"),
                (dict(flat=ctypes.c_void_p((8 << 32) + 799)), b"alias"), (dict(order=ctypes.c_void_p((2 << 32) + 72)), b"alias")])
    # what is not an error: no sums; no points -- and nothing is launched or written for them
    assert lib.d3d_cloud_normals(None, None, None, 0, 16, 8, 4, 0.5, 0, P(4), need, None, None, None, None, None) == 0
    assert lib.d3d_cloud_normals(None, None, None, 0, 16, 8, 4, 0.5, 1, None, need, None, None, None, None, None) == -1


def test_the_operator_refuses_cpu_tensors_bad_dtypes_and_settings():
    b = [0, 4, 0, 4, 0, 4]
    xyz = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CN.estimate(xyz, b, 1.0)
    for bad in (xyz.double(), torch.zeros(5, 2), torch.zeros(15)):
        with pytest.raises(ValueError, match="xyz"):
            CN.estimate(bad, b, 1.0)
    with pytest.raises(TypeError, match="Tensor"):
        CN.estimate(np.zeros((5, 3), np.float32), b, 1.0)
    for kw, msg in ((dict(radius=0.0), "voxel"), (dict(radius=math.nan), "voxel"), (dict(radius=1e-9), "2\\^21"), (dict(border=[0, 4, 0, 4]), "six"),
                    (dict(z_down=1), "z_down"), (dict(z_down=None), "z_down"), (dict(return_sums="yes"), "return_sums")):
        with pytest.raises(ValueError, match=msg):
            CN.estimate(**dict(dict(xyz=xyz, border=b, radius=1.0), **kw))


def test_the_kernel_uses_no_atomics_the_shared_search_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/cloud_normals.hip").read())
    assert not re.search(r"atomic|__shfl|\basm\b|fma\b", hip)
    assert '#include "cloud_search.h"' in hip and all(c in hip for c in ("search_tile(", "search_walk(", "search_gather(", "search_apart(", "count_ok("))
    assert not re.search(r"\bbound\[|keys\[mid\]", hip)                       # the search itself is not restated
    assert not re.search(r"\[\s*(sweep|i|j|k|r|c)\s*\]", hip)                 # no array indexed at run time: named registers only
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bcloud_normals\.hip\b", make, re.M) and "-ffp-contract=off" in make


# ----------------------------------------------------------------------------------------
# files and the command line
# ----------------------------------------------------------------------------------------
def test_the_ply_reader_returns_normals_where_the_file_has_them(tmp_path):
    rng = np.random.default_rng(0)
    xyz, nrm = rng.uniform(0, 4, (7, 3)).astype(np.float32), rng.standard_normal((7, 3)).astype(np.float32)
    col = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    for color in (None, col):
        path = tmp_path / ("n%d.ply" % (color is not None))
        path.write_bytes(CN.normals_ply_bytes(xyz, nrm, color))
        assert np.array_equal(CC.read_xyz_ply(path), xyz)                              # existing callers get what they got
        got = CC.read_xyz_ply(path, normals=True)
        assert np.array_equal(got[0], xyz) and np.array_equal(got[1], nrm) and got[1].dtype == np.float32 and got[1].flags.c_contiguous
        rec = CC.read_vertex_ply(path)
        assert rec.dtype.names == ("x", "y", "z", "nx", "ny", "nz") + (("red", "green", "blue") if color is not None else ())
        if color is not None:
            assert np.array_equal(CC.vertex_columns(rec, ("red", "green", "blue"), np.uint8), col)
    from deep3d_aerial_amd import cloud_register as CR

    bare = tmp_path / "bare.ply"
    bare.write_bytes(CR.xyz_ply_bytes(xyz))
    assert CC.read_xyz_ply(bare, normals=True)[1] is None
    # the merged cloud's own layout carries normals too; two of the three are not normals
    merged = tmp_path / "merged.ply"
    cloud.write_cloud_ply(merged, xyz, nrm, col, np.ones(7, np.int32))
    assert np.array_equal(CC.read_xyz_ply(merged, normals=True)[1], nrm)
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nend_header\n"
    (tmp_path / "two.ply").write_bytes(head + np.zeros(5, "<f4").tobytes())
    assert CC.read_xyz_ply(tmp_path / "two.ply", normals=True)[1] is None
    with pytest.raises(ValueError, match="float32"):
        CN.normals_ply_bytes(xyz, nrm.astype(np.float64))
    with pytest.raises(ValueError, match="color"):
        CN.normals_ply_bytes(xyz, nrm, col[:5])


def test_the_command_line_refuses_bad_settings_before_any_gpu_work(capsys, tmp_path):
    base = ["--cloud", str(tmp_path / "a.ply"), "--out", str(tmp_path / "b.ply"), "--border=0,4,0,4,0,4", "--radius=1.0"]
    for argv, msg in ((base[:4] + base[5:], "--border is required"), (base[:5], "--radius is required"),
                      (base[:3] + [str(tmp_path / "b.txt")] + base[4:], "must end in .ply"), (base[:5] + ["--radius=0"], "voxel"),
                      (base + ["--min_count=-1"], "min_count"), (base[:4] + ["--border=0,4,0,4", "--radius=1.0"], "border")):
        with pytest.raises(SystemExit):
            CN.main(argv)
        assert msg in capsys.readouterr().err, argv
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CN.main(base)
