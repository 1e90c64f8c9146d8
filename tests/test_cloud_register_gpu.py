"""The registration of a point cloud to a reference on the GPU (csrc/cloud_register.hip, cloud_register.apply / pair_sums /
register): the transform and the 27 sums bit-equal to the numpy restatement of tests/cloud_register_scene.py -- at every size
around a lane's four points, a wave and a workgroup, on an unaligned view, on large coordinates, on non-finite ones, on more pairs
than one pass of the largest launch, on pairs that do not count, in the far corner of the largest grid --; register() equal to the
restated iteration in T, the log and the moved cloud (if the sums are bit-equal everything after them is the same host code, so a
mismatch points at a kernel); and the file tools, --transform of the two compare tools included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_register_scene as S
import test_cloud as TC
import test_cloud_compare as TCC
import test_cloud_register as TCR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRID_CAP = 2048   # CR_GRID_CAP of csrc/cloud_register.hip: the workgroups launched at most, 256 lanes each


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 3)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _motion(seed=0, shift=(0.25, -0.2, 0.15)):
    rng = np.random.default_rng(seed)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, shift
    return T


# ----------------------------------------------------------------------------------------
# apply
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1025])
def test_apply_at_sizes_around_a_lane_a_wave_and_a_workgroup(n):
    from deep3d_aerial_amd import cloud_register as CR

    xyz = np.random.default_rng(n).uniform(-50, 50, (n, 3)).astype(np.float32)
    T = _motion(n)
    d = _cuda(xyz)
    got = CR.apply(d, T)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, 3) and (n == 0 or got.data_ptr() != d.data_ptr())
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(S.transform_numpy(xyz, T)))
    assert np.array_equal(d.cpu().numpy(), xyz)                     # the input is left alone
    assert torch.equal(CR.apply(d, np.eye(4)), d)                   # the identity is exact


def test_apply_on_an_unaligned_view_large_coordinates_and_non_finite_ones():
    from deep3d_aerial_amd import cloud_register as CR

    rng = np.random.default_rng(1)
    xyz = rng.uniform(-50, 50, (1030, 3)).astype(np.float32)
    T = _motion(1)
    d = _cuda(xyz)
    for skip in (1, 2, 3):   # a view that starts 12, 24, 36 bytes into the allocation: no 16-byte loads
        view = d[skip:]
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        assert np.array_equal(_bits(CR.apply(view, T).cpu().numpy()), _bits(S.transform_numpy(xyz[skip:], T)))
    assert np.array_equal(_bits(CR.apply(d[4:], T).cpu().numpy()), _bits(S.transform_numpy(xyz[4:], T)))   # 48 bytes in: aligned again
    # coordinates near 5e5 (an fp32 ulp there is 1/32) with a rotation: the fp64 products are rounded once each
    big = (rng.uniform(-100, 100, (777, 3)) + [5e5, 4.8e5, 300]).astype(np.float32)
    Tb = _motion(2, (-4e5, 1e5, 7.0))
    assert np.array_equal(_bits(CR.apply(_cuda(big), Tb).cpu().numpy()), _bits(S.transform_numpy(big, Tb)))
    # NaN and inf go through the arithmetic as it is: inf times 0 is NaN, inf minus inf too
    odd = np.float32([[np.nan, 1, 2], [np.inf, 1, 2], [1, -np.inf, 2], [np.inf, np.inf, 1], [3e38, 3e38, 3e38], [1, 2, 3], [-0.0, 0.0, -0.0]])
    for To in (np.eye(4), _motion(3), np.array([[0, 1, 0, 0], [1, 0, 0, 0], [1, -1, 1, 0], [0, 0, 0, 1.0]]), np.diag([2.0, 2.0, 2.0, 1.0])):
        got, want = CR.apply(_cuda(odd), To).cpu().numpy(), S.transform_numpy(odd, To)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)])
    assert np.isnan(S.transform_numpy(odd, np.eye(4))[1]).any() and np.isinf(S.transform_numpy(odd, np.diag([2.0, 2.0, 2.0, 1.0]))[4]).all()


# ----------------------------------------------------------------------------------------
# pair_sums
# ----------------------------------------------------------------------------------------
def _pairs(n, m, seed, grid):
    """n moved points and m reference points inside the grid with made-up e and idx: about a tenth of the pairs has idx = -1,
    and e spreads over 0 .. 1024.  The sums do not ask whether e and idx come from a search."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(grid.border[0::2]), np.array(grid.border[1::2])
    moved = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    ref = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    idx = np.where(rng.uniform(size=n) < 0.1, -1, rng.integers(0, max(m, 1), n)).astype(np.int32)
    e = rng.integers(0, 1025, n).astype(np.int32)
    return moved, e, idx, ref


def _check_sums(moved, e, idx, ref, grid, e_max=1024):
    from deep3d_aerial_amd import cloud_register as CR

    got = CR.pair_sums(_cuda(moved), torch.from_numpy(e).cuda(), torch.from_numpy(idx).cuda(), _cuda(ref), grid, e_max)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (27,)
    want = S.sums_numpy(moved, e, idx, ref, grid, e_max)
    assert got.tolist() == want
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_pair_sums_at_sizes_around_a_wave_and_a_workgroup(n):
    g = TC.unit_grid(40, 30, 9)
    moved, e, idx, ref = _pairs(n, 91, n, g)
    w = _check_sums(moved, e, idx, ref, g)
    assert w[0] == (idx >= 0).sum()
    # under a permutation of the queries: the same bits
    p = np.random.default_rng(n + 1).permutation(n)
    assert _check_sums(moved[p], e[p], idx[p], ref, g) == w
    # no reference at all: nothing counts
    assert _check_sums(moved, e, np.full(n, -1, np.int32), ref[:0], g) == [0] * 27


def test_pair_sums_on_more_pairs_than_one_pass_of_the_largest_launch():
    n = 256 * GRID_CAP + 257
    assert n == 524545
    from deep3d_aerial_amd import cloud

    g = cloud.CloudGrid([-3.0, 97.0, 10.0, 110.0, 0.0, 12.5], 0.25)
    moved, e, idx, ref = _pairs(n, 5000, 7, g)
    w = _check_sums(moved, e, idx, ref, g, 700)
    assert n // 2 < w[0] < n * 3 // 4


def test_pairs_that_do_not_count_and_the_values_of_e_max():
    g = TC.unit_grid(12, 12, 12)
    n = 1500
    moved, e, idx, ref = _pairs(n, 300, 3, g)
    assert _check_sums(moved, e, np.full(n, -1, np.int32), ref, g) == [0] * 27                  # idx = -1 everywhere
    assert _check_sums(moved, np.full(n, 501, np.int32), idx, ref, g, 500) == [0] * 27           # e above e_max everywhere
    e[:200] = np.repeat(np.int32([0, 1, 2, 1024]), 50)
    counts = [_check_sums(moved, e, idx, ref, g, e_max)[0] for e_max in (0, 1, 1024)]
    assert 0 < counts[0] < counts[1] < counts[2] == (idx >= 0).sum()
    # an idx outside the reference on a pair that would count: ignored (the restatement ignores it too), and nothing faults
    idx2 = idx.copy()
    idx2[::7] = np.resize(np.int32([300, 301, 1 << 20, 2 ** 31 - 1, -2, -(2 ** 31)]), len(idx2[::7]))
    w = _check_sums(moved, e, idx2, ref, g)
    assert w[0] == ((idx2 >= 0) & (idx2 < 300)).sum() < counts[2]


def test_the_far_corner_of_the_largest_grid_where_a_plain_sum_wraps():
    moved, e, idx, ref, g = TCR.far_corner()
    w = _check_sums(moved, e, idx, ref, g)
    assert w[0] == 8 and min(w[16:25]) > 1 << 32            # the high limbs alone are past 32 bits' worth of 2^32
    # and through the search itself: every point finds its partner a quarter or three eighths of a cell away
    from deep3d_aerial_amd import cloud_compare as CC, cloud_register as CR

    e2, idx2, _ = CC.nearest(_cuda(moved), _cuda(ref), g)
    want = TCC.nearest_numpy(moved, ref, g)
    assert np.array_equal(e2.cpu().numpy(), want[0]) and np.array_equal(idx2.cpu().numpy(), want[1]) and (want[1] >= 0).all()
    assert CR.pair_sums(_cuda(moved), e2, idx2, _cuda(ref), g).tolist() == S.sums_numpy(moved, want[0], want[1], ref, g)


# ----------------------------------------------------------------------------------------
# register
# ----------------------------------------------------------------------------------------
def _same(got, want):
    T, log, moved = got
    assert isinstance(T, np.ndarray) and T.dtype == np.float64 and T.shape == (4, 4)
    assert T.tobytes() == np.ascontiguousarray(want[0]).tobytes()
    assert log == want[1]
    assert moved.is_cuda and np.array_equal(_bits(moved.cpu().numpy()), _bits(want[2]))


@pytest.mark.parametrize("separate", [False, True], ids=["same_points", "separate_samples"])
@pytest.mark.parametrize("caps", [(1.0,), (1.0, 0.5)], ids=str)
def test_register_is_the_restated_iteration_on_the_scene(separate, caps):
    from deep3d_aerial_amd import cloud_register as CR

    p, q, truth = S.scene(separate)
    want = S.registered(separate, caps)
    _same(CR.register(_cuda(p), _cuda(q), S.BORDER, list(caps)), want)
    assert S.corner_error(want[0], truth) < (TCR.SEPARATE_BOUND if separate else TCR.SAME_POINTS_BOUND[caps])


def test_register_with_one_iteration_a_solving_init_a_degenerate_start_and_a_pair_cap():
    from deep3d_aerial_amd import cloud_register as CR

    p, q, _ = S.scene(False)
    dp, dq = _cuda(p), _cuda(q)
    got = CR.register(dp, dq, S.BORDER, [1.0], max_iterations=1)
    _same(got, S.register_numpy(p, q, S.BORDER, [1.0], max_iterations=1))
    assert len(got[1]) == 1 and got[1][0]["reason"] == "iterations"
    solved = S.registered(False, (1.0,))[0]
    got = CR.register(dp, dq, S.BORDER, [1.0], init=solved)
    _same(got, S.register_numpy(p, q, S.BORDER, [1.0], init=solved))
    assert len(got[1]) == 1 and got[1][0]["reason"] == "converged"
    far = (p + np.float32([0, 0, 4.5])).astype(np.float32)      # out of the reference's reach: the first iteration is degenerate
    got = CR.register(_cuda(far), dq, S.BORDER, [1.0, 0.5])
    _same(got, S.register_numpy(far, q, S.BORDER, [1.0, 0.5]))
    assert [e["reason"] for e in got[1]] == ["degenerate"] * 2 and np.array_equal(got[0], np.eye(4))
    got = CR.register(dp, dq, S.BORDER, [1.0], max_pair_dist=0.4, max_iterations=3, tolerance=1e-3)
    _same(got, S.register_numpy(p, q, S.BORDER, [1.0], max_pair_dist=0.4, max_iterations=3, tolerance=1e-3))
    # an empty cloud and an empty reference are degenerate, not an error
    none = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    for a, b in ((none, dq), (dp, none), (none, none)):
        T, log, moved = CR.register(a, b, S.BORDER, [1.0])
        assert np.array_equal(T, np.eye(4)) and [e["reason"] for e in log] == ["degenerate"] and log[0]["pairs"] == 0 and moved.shape == a.shape




# ----------------------------------------------------------------------------------------
# the file tools
# ----------------------------------------------------------------------------------------
def _scene_files(tmp_path):
    from deep3d_aerial_amd import cloud_register as CR

    p, q, _ = S.scene(False)
    (tmp_path / "a.ply").write_bytes(CR.xyz_ply_bytes(p))
    (tmp_path / "b.ply").write_bytes(CR.xyz_ply_bytes(q))
    return str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--border=%s" % ",".join(repr(v) for v in S.BORDER)


def test_the_file_tool_writes_the_transform_the_log_and_the_registered_cloud(tmp_path):
    """The module run as a program (one child process: the test is about the command line)."""
    from deep3d_aerial_amd import cloud_compare as CC, cloud_register as CR

    a, b, border = _scene_files(tmp_path)
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.cloud_register", "--cloud", a, "--reference", b, border, "--max_dist=1.0",
           "--out_transform", str(out / "T.txt"), "--out", str(out / "a_registered.ply"), "--json", str(out / "log.json")]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1
    res = json.loads(lines[0])
    want = S.registered(False, (1.0,))
    assert CR.read_transform(out / "T.txt").tobytes() == np.ascontiguousarray(want[0]).tobytes()
    assert res["transform"] == want[0].tolist() and res["log"] == want[1] and res["iterations"] == len(want[1]) and res["stages"] == [want[1][-1]]
    assert res == json.loads((out / "log.json").read_text())
    assert np.array_equal(_bits(CC.read_xyz_ply(out / "a_registered.ply")), _bits(want[2]))


def test_the_compare_tools_move_the_evaluated_side_by_the_transform_first(tmp_path, capsys):
    """cloud_compare --transform T.txt prints what compare() gives on apply(P, T), mesh_compare --transform what its compare() gives on
    the moved vertices; the --out_* files carry the moved coordinates; and the F-score at an eighth of the cap rises from below
    0.5 to above 0.9 (bounds the restatement clears on the CPU: tests/test_cloud_register.py)."""
    from deep3d_aerial_amd import cloud_compare as CC, cloud_register as CR, mesh, mesh_compare as MC

    a, b, border = _scene_files(tmp_path)
    p, q, truth = S.scene(False)
    out = tmp_path / "out"
    T = CR.read_transform(CR.write_transform(out / "T.txt", S.registered(False, (1.0,))[0]))
    h, tau = 1.0, 0.125

    def tool(main, argv):
        capsys.readouterr()
        result = main(argv)
        lines = capsys.readouterr().out.strip().split("\n")
        assert len(lines) == 1 and json.loads(lines[0]) == result
        return json.loads(lines[0])

    args = ["--cloud", a, "--reference", b, border, "--max_dist=%r" % h, "--threshold=%r" % tau]
    after = tool(CC.main, args + ["--transform", str(out / "T.txt"), "--out_accuracy", str(out / "ea.ply")])
    moved = CR.apply(_cuda(p), T)
    result, found = CC.compare(moved, _cuda(q), S.BORDER, h, [tau])
    assert after == result and (out / "ea.ply").read_bytes() == CC.error_cloud_bytes(moved, found["cloud"][0])
    before = tool(CC.main, args)
    assert before == CC.compare(_cuda(p), _cuda(q), S.BORDER, h, [tau])[0]
    print("fscore at %r: %.4f unregistered, %.4f registered" % (tau, before["thresholds"][0]["fscore"], after["thresholds"][0]["fscore"]))
    assert before["thresholds"][0]["fscore"] < 0.5 and after["thresholds"][0]["fscore"] > 0.9
    # a small mesh of the moved surface: 16 x 16 squares, two triangles each
    k = np.arange(17) * 1.6 + 3.2
    gx, gy = np.meshgrid(k, k, indexing="ij")
    M = np.linalg.inv(truth)
    v = (np.stack([gx, gy, S.height(gx, gy)], -1).reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    c = (np.arange(16)[:, None] * 17 + np.arange(16)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([c, c + 17, c + 1], 1), np.stack([c + 1, c + 17, c + 18], 1)]).astype(np.int32)
    mesh.write_ply(str(tmp_path / "m.ply"), v, f)
    margs = ["--mesh", str(tmp_path / "m.ply"), "--reference", b, border, "--max_dist=%r" % h, "--threshold=0.25", "--spacing=0.4"]
    mafter = tool(MC.main, margs + ["--transform", str(out / "T.txt"), "--out_samples", str(out / "s.ply")])
    dv = CR.apply(_cuda(v), T)
    mresult, mfound = MC.compare(dv, torch.from_numpy(f).cuda(), _cuda(q), S.BORDER, h, [0.25], 0.4)
    assert mafter == mresult and (out / "s.ply").read_bytes() == MC.samples_bytes(mfound["samples"][0], mfound["samples"][1])
    assert tool(MC.main, margs)["thresholds"][0]["accuracy"] < mafter["thresholds"][0]["accuracy"]
