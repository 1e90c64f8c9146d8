"""The point-to-plane metric of the registration on the GPU (csrc/cloud_register.hip, cloud_register.plane_sums and
register(metric="plane")): the 87 sums bit-equal to the restatement of tests/test_cloud_register_plane.py -- at no pair, one, 300,
with negative products, with normals and indices that do not count, in the far corner of the largest grid, on more pairs than one
pass of the largest launch, under a permutation --; register() end to end against the point metric on the scene of
tests/cloud_register_scene.py; and the file tools."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_register_scene as S
import test_cloud as TC
import test_cloud_register as TCR
import test_cloud_register_plane as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRID_CAP = 2048   # CR_GRID_CAP of csrc/cloud_register.hip: the workgroups launched at most, 256 lanes each
NORMAL_RADIUS = 3 * S.SPACING


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 3)).cuda()


def _pairs(n, m, seed, grid):
    """n moved points, m reference points with unit normals of every sign, made-up e and idx (a tenth of them -1)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(grid.border[0::2]), np.array(grid.border[1::2])
    moved = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    ref = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    nrm = rng.standard_normal((m, 3))
    nrm = (nrm / np.sqrt((nrm * nrm).sum(1))[:, None]).astype(np.float32)
    idx = np.where(rng.uniform(size=n) < 0.1, -1, rng.integers(0, max(m, 1), n)).astype(np.int32)
    e = rng.integers(0, 1025, n).astype(np.int32)
    return moved, e, idx, ref, nrm


def _check_sums(moved, e, idx, ref, nrm, grid, e_max=1024):
    from deep3d_aerial_amd import cloud_register as CR

    got = CR.plane_sums(_cuda(moved), torch.from_numpy(e).cuda(), torch.from_numpy(idx).cuda(), _cuda(ref), _cuda(nrm), grid, e_max)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (87,)
    want = TP.plane_sums_numpy(moved, e, idx, ref, nrm, grid, e_max)
    assert got.tolist() == want
    return want


@pytest.mark.parametrize("n", [0, 1, 300])
def test_plane_sums_at_no_pair_one_pair_and_300_with_a_permutation(n):
    g = TC.unit_grid(40, 30, 9)
    moved, e, idx, ref, nrm = _pairs(n, 91, n, g)
    if n == 1:
        idx[0] = 5
    w = _check_sums(moved, e, idx, ref, nrm, g)
    assert w[0] == (idx >= 0).sum()
    if n == 300:
        assert min(w[5::3]) < 0 < max(w[3::3])                       # negative products among them: a high word of -1 each
    p = np.random.default_rng(n + 1).permutation(n)
    assert _check_sums(moved[p], e[p], idx[p], ref, nrm, g) == w    # the same bits in another order
    assert _check_sums(moved, e, np.full(n, -1, np.int32), ref[:0], nrm[:0], g) == [0] * 87


def test_normals_and_indices_that_do_not_count():
    g = TC.unit_grid(12, 12, 12)
    n = 1500
    moved, e, idx, ref, nrm = _pairs(n, 300, 3, g)
    nrm[::5] = np.resize(np.float32([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [0, 0, -1.5], [2e-4, -3e-4, 1e-4], [0, 0, -0.0]]), nrm[::5].shape)
    w = _check_sums(moved, e, idx, ref, nrm, g)
    assert 0 < w[0] < (idx >= 0).sum()
    assert _check_sums(moved, e, np.full(n, -1, np.int32), ref, nrm, g) == [0] * 87
    assert _check_sums(moved, np.full(n, 501, np.int32), idx, ref, nrm, g, 500) == [0] * 87
    assert _check_sums(moved, e, idx, ref, np.zeros_like(nrm), g) == [0] * 87
    idx2 = idx.copy()
    idx2[::7] = np.resize(np.int32([300, 301, 1 << 20, 2 ** 31 - 1, -2, -(2 ** 31)]), len(idx2[::7]))
    assert _check_sums(moved, e, idx2, ref, nrm, g)[0] < w[0]           # an idx outside the reference is ignored, and nothing faults
    counts = [_check_sums(moved, e, idx, ref, nrm, g, e_max)[0] for e_max in (0, 400, 1024)]
    assert counts[0] < counts[1] < counts[2] == w[0]


def test_the_far_corner_of_the_largest_grid_where_the_high_limb_is_in_use():
    moved, e, idx, ref, g = TCR.far_corner()
    assert max(g.n) == (1 << 21) - 1
    nrm = np.resize(np.float32([[1, 0, 0], [-0.6, 0.8, 0], [0, -1, 0], [0.577, 0.577, -0.577]]), ref.shape)
    w = _check_sums(moved, e, idx, ref, nrm, g)
    assert w[0] == 8 and max(abs(v) for v in w[5::3]) > 1 << 12       # products past 2^76: the signed high words carry them


def test_plane_sums_on_more_pairs_than_one_pass_of_the_largest_launch():
    n = 600000
    assert n > 256 * GRID_CAP
    from deep3d_aerial_amd import cloud

    g = cloud.CloudGrid([-3.0, 97.0, 10.0, 110.0, 0.0, 12.5], 0.25)
    moved, e, idx, ref, nrm = _pairs(n, 5000, 7, g)
    w = _check_sums(moved, e, idx, ref, nrm, g, 700)
    assert n // 2 < w[0] < n * 3 // 4


# ----------------------------------------------------------------------------------------
# register
# ----------------------------------------------------------------------------------------
CAPS = (1.0, 0.5)   # the schedule of tests/test_cloud_register_gpu.py


def test_the_point_metric_is_untouched_by_the_new_arguments():
    from deep3d_aerial_amd import cloud_register as CR

    p, q, _ = S.scene(True)
    dp, dq = _cuda(p), _cuda(q)
    T0, log0, m0 = CR.register(dp, dq, S.BORDER, list(CAPS))
    T1, log1, m1 = CR.register(dp, dq, S.BORDER, list(CAPS), metric="point", reference_normals=None, normal_radius=None, z_down=False)
    assert T0.tobytes() == T1.tobytes() == np.ascontiguousarray(S.registered(True, CAPS)[0]).tobytes()
    assert log0 == log1 and torch.equal(m0.view(torch.int32), m1.view(torch.int32))
    assert all("plane_rms" not in entry and "rank" not in entry for entry in log0)


def test_plane_ends_closer_than_point_on_a_separately_drawn_sample():
    """corner_error on scene(separate=True), caps (1.0, 0.5), normals estimated at three spacings: strictly smaller with the
    plane metric than with the point metric in the same run, and below the point spacing.  Measured on an MI355X: point 0.1442
    after 45 iterations, plane 0.0024 after 5 (spacing 0.5)."""
    from deep3d_aerial_amd import cloud_register as CR

    p, q, truth = S.scene(True)
    dp, dq = _cuda(p), _cuda(q)
    point = CR.register(dp, dq, S.BORDER, list(CAPS))
    plane = CR.register(dp, dq, S.BORDER, list(CAPS), metric="plane", normal_radius=NORMAL_RADIUS)
    ep, el = S.corner_error(point[0], truth), S.corner_error(plane[0], truth)
    print("corner error: point %.4f, plane %.4f (spacing %.2f); iterations %d and %d; last plane entry %r"
          % (ep, el, S.SPACING, len(point[1]), len(plane[1]), plane[1][-1]))
    assert el < ep and el < S.SPACING
    assert all(entry["rank"] == 6 for entry in plane[1])
    assert sorted(plane[1][0]) == ["cap", "iteration", "moved", "pairs", "plane_rms", "rank", "rms", "stage"]
    # two runs: the same bits; given normals: the same as estimating them
    from deep3d_aerial_amd import cloud_normals as CN

    again = CR.register(dp, dq, S.BORDER, list(CAPS), metric="plane", reference_normals=CN.estimate(dq, S.BORDER, NORMAL_RADIUS)[0])
    assert again[0].tobytes() == plane[0].tobytes() and again[1] == plane[1]
    assert torch.equal(again[2].view(torch.int32), plane[2].view(torch.int32))


def test_plane_reaches_what_point_reaches_on_the_same_points():
    from deep3d_aerial_amd import cloud_register as CR

    p, q, truth = S.scene(False)
    dp, dq = _cuda(p), _cuda(q)
    ep = S.corner_error(S.registered(False, CAPS)[0], truth)
    plane = CR.register(dp, dq, S.BORDER, list(CAPS), metric="plane", normal_radius=NORMAL_RADIUS)
    el = S.corner_error(plane[0], truth)
    print("corner error on the same points: point %.3g, plane %.3g" % (ep, el))
    assert el < 10 * ep
    empty = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    for a, b in ((empty, dq), (dp, empty)):                            # nothing to pair: degenerate, not an error
        T, log, moved = CR.register(a, b, S.BORDER, [1.0], metric="plane", normal_radius=NORMAL_RADIUS)
        assert np.array_equal(T, np.eye(4)) and [e["reason"] for e in log] == ["degenerate"] and log[0]["pairs"] == 0 and log[0]["rank"] == 0


def test_the_file_tool_with_the_plane_metric_and_the_compare_tool_after_it(tmp_path, capsys):
    """The module run as a program (one child process: the test is about the command line), with the reference's own normals
    from its file; then in-process with --normal_radius, and cloud_compare --transform on what it wrote."""
    from deep3d_aerial_amd import cloud_compare as CC, cloud_normals as CN, cloud_register as CR

    p, q, truth = S.scene(True)
    normals = CN.estimate(_cuda(q), S.BORDER, NORMAL_RADIUS)[0]
    (tmp_path / "a.ply").write_bytes(CR.xyz_ply_bytes(p))
    (tmp_path / "b.ply").write_bytes(CN.normals_ply_bytes(q, normals))
    (tmp_path / "bare.ply").write_bytes(CR.xyz_ply_bytes(q))
    border = "--border=%s" % ",".join(repr(v) for v in S.BORDER)
    out = tmp_path / "out"
    args = ["--cloud", str(tmp_path / "a.ply"), border, "--max_dist=1.0,0.5", "--metric", "plane"]
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.cloud_register"] + args + ["--reference", str(tmp_path / "b.ply"), "--out_transform",
                                                                                 str(out / "T.txt"), "--json", str(out / "log.json")]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip())
    want = CR.register(_cuda(p), _cuda(q), S.BORDER, list(CAPS), metric="plane", reference_normals=normals)
    T = CR.read_transform(out / "T.txt")
    assert T.tobytes() == want[0].tobytes() and res["transform"] == want[0].tolist() and res["log"] == want[1]
    assert res == json.loads((out / "log.json").read_text())
    capsys.readouterr()
    res2 = CR.main(args + ["--reference", str(tmp_path / "bare.ply"), "--normal_radius=%r" % NORMAL_RADIUS, "--out_transform", str(out / "T2.txt")])
    assert res2["transform"] == want[0].tolist() and CR.read_transform(out / "T2.txt").tobytes() == T.tobytes()
    with pytest.raises(ValueError, match="no nx ny nz"):
        CR.main(args + ["--reference", str(tmp_path / "bare.ply")])
    capsys.readouterr()
    cargs = ["--cloud", str(tmp_path / "a.ply"), "--reference", str(tmp_path / "b.ply"), border, "--max_dist=1.0", "--threshold=0.125"]
    after = CC.main(cargs + ["--transform", str(out / "T.txt")])
    assert after == CC.compare(CR.apply(_cuda(p), T), _cuda(q), S.BORDER, 1.0, [0.125])[0]
    before = CC.main(cargs)
    capsys.readouterr()
    assert before["thresholds"][0]["fscore"] < after["thresholds"][0]["fscore"]
