"""CPU checks of the registration of a point cloud to a reference (deep3d_aerial_amd/cloud_register.py, csrc/cloud_register.hip,
DESIGN.md §4.31): solve() on hand-made sums, why the sums are split into 32-bit limbs, the numpy restatement of
tests/cloud_register_scene.py on its scene, what the order of either cloud changes, the transform file, the command lines' refusals
(--transform of the two compare tools included), the C ABI and its argument checks, and the sources.
tests/test_cloud_register_gpu.py compares the kernels against the restatement bit for bit."""
import ctypes
import itertools
import math
import re

import numpy as np
import pytest
import torch

import cloud_register_scene as S
import test_cloud as TC
import test_cloud_compare as TCC
from deep3d_aerial_amd import _lib, cloud, cloud_compare as CC, cloud_register as CR, mesh_compare as MC

NEW_SYMBOLS = ("d3d_cloud_transform", "d3d_cloud_register_sums")

# What register_numpy measured on the scene, with the same points on both sides (the largest corner error against the truth):
# 3.03e-5 after the cap 1.0 (6 iterations) and 5.96e-6 after the schedule 1.0, 0.5 (7).  The result is determined by the fp32
# rounding of the coordinates; the bound is 16 times the measured value, which leaves room for another BLAS's SVD.
SAME_POINTS_BOUND = {(1.0,): 16 * 3.03e-5, (1.0, 0.5): 16 * 5.96e-6}
# With a separately drawn sample as the evaluated cloud the nearest reference point is not the same surface point, and the answer is
# off by a fraction of the point spacing: half the spacing is the bound (measured: 0.148 after 37 iterations at the cap 1.0, 0.144
# after 45 with the schedule 1.0, 0.5).
SEPARATE_BOUND = 0.5 * S.SPACING


def sums_of(a, b, e=None):
    """The 27 sums of hand-made integer pairs."""
    e = [0] * len(a) if e is None else e
    prod = [[sum(x[r] * y[c] for x, y in zip(a, b)) for c in range(3)] for r in range(3)]
    assert all(0 <= x[r] * y[c] for x, y in zip(a, b) for r in range(3) for c in range(3))
    lo = [sum((x[r] * y[c]) & 0xFFFFFFFF for x, y in zip(a, b)) for r in range(3) for c in range(3)]
    hi = [sum((x[r] * y[c]) >> 32 for x, y in zip(a, b)) for r in range(3) for c in range(3)]
    assert [(h << 32) + l for h, l in zip(hi, lo)] == [prod[r][c] for r in range(3) for c in range(3)]
    return ([len(a)] + [sum(x[c] for x in a) for c in range(3)] + [sum(y[c] for y in b) for c in range(3)] + lo + hi
            + [sum(e), sum(v * v for v in e)])


# ----------------------------------------------------------------------------------------
# solve
# ----------------------------------------------------------------------------------------
A_POINTS = [(1024, 2048, 512), (9000, 100, 3000), (4096, 8192, 7000), (300, 5000, 1000), (7777, 3333, 5555), (2000, 2000, 100)]


def test_solve_a_translation_by_whole_bins():
    g = cloud.CloudGrid([-3.0, 13.0, 2.0, 18.0, 0.0, 8.0], 0.5)
    shift = (2048, -1024, 512)   # bins: (1.0, -0.5, 0.25) world units at the cap 0.5
    a = [tuple(v + 4096 for v in p) for p in A_POINTS]
    b = [tuple(v + s for v, s in zip(p, shift)) for p in a]
    dT, info = CR.solve(sums_of(a, b, [3, 4, 0, 0, 5, 0]), g)
    assert info == {"pairs": 6, "rms": math.sqrt(50 / 6) / 1024 * 0.5, "degenerate": False}
    assert dT.dtype == np.float64 and dT.shape == (4, 4) and dT[3].tolist() == [0, 0, 0, 1]
    assert np.abs(dT[:3, :3] - np.eye(3)).max() < 1e-14
    assert np.abs(dT[:3, 3] - [1.0, -0.5, 0.25]).max() < 1e-11   # (the means are near 10; the rotation's 1e-15 moves them that much)
    assert abs(CR.corner_motion(dT, g.border) - math.sqrt(1.0 + 0.25 + 0.0625)) < 1e-11
    # a torch tensor and a numpy array serve as well as a list
    for other in (torch.tensor(sums_of(a, b)), np.array(sums_of(a, b))):
        assert np.array_equal(CR.solve(other, g)[0], CR.solve(sums_of(a, b), g)[0])
    with pytest.raises(ValueError, match="27"):
        CR.solve([0] * 26, g)
    with pytest.raises(TypeError, match="CloudGrid"):
        CR.solve([0] * 27, None)


def test_solve_a_rotation_about_z():
    g = TC.unit_grid(16, 16, 16)
    c = 8192
    a = [tuple(v + c for v in p) for p in ((1000, 0, 0), (0, 2000, 0), (0, 0, 3000), (-1000, -500, 200), (700, 700, -900))]
    b = [(2 * c - p[1], p[0], p[2]) for p in a]   # a quarter turn about the vertical through (c, c): (x, y) -> (-y, x)
    dT, info = CR.solve(sums_of(a, b), g)
    assert not info["degenerate"] and np.abs(dT[:3, :3] - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-14
    assert np.abs(dT[:3, 3] - [16.0, 0.0, 0.0]).max() < 1e-11


@pytest.mark.parametrize("n", [0, 1, 2])
def test_fewer_than_three_pairs_are_degenerate(n):
    dT, info = CR.solve(sums_of(A_POINTS[:n], A_POINTS[1:n + 1]), TC.unit_grid(16, 16, 16))
    assert dT is None and info == {"pairs": n, "rms": 0.0, "degenerate": True}


def test_collinear_points_are_degenerate_and_a_mirror_gives_a_proper_rotation():
    g = TC.unit_grid(16, 16, 16)
    line = [(100 + 3 * k, 200 + 5 * k, 50 + 7 * k) for k in (0, 1, 2, 5, 9, 40)]
    dT, info = CR.solve(sums_of(line, [(x + 10, y, z + 3) for x, y, z in line]), g)
    assert dT is None and info["degenerate"] and info["pairs"] == 6
    same = [(500, 500, 500)] * 5   # one position five times: no spread at all
    assert CR.solve(sums_of(same, same), g)[0] is None
    # the reference is the mirror image of the cloud: the least-squares ORTHOGONAL map is the reflection; the solve gives a rotation
    mirror = [(10000 - x, y, z) for x, y, z in A_POINTS]
    dT, info = CR.solve(sums_of(A_POINTS, mirror), g)
    R = dT[:3, :3]
    assert not info["degenerate"] and abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert np.abs(R - np.diag([-1.0, 1.0, 1.0])).max() > 0.5


# ----------------------------------------------------------------------------------------
# the split limbs
# ----------------------------------------------------------------------------------------
def far_corner():
    """(moved, e, idx, reference, grid): eight pairs in the far corner of a grid with 2^21 - 1 cells per axis."""
    n = (1 << 21) - 1
    g = cloud.CloudGrid([0.0, float(n), 0.0, float(n), 0.0, float(n)], 1.0)
    assert g.n == (n, n, n)
    k = np.arange(8)
    moved = np.float32(n) - np.stack([0.25 + 0.25 * (k & 1), 0.25 + 0.25 * (k >> 1 & 1), 0.25 + 0.25 * (k >> 2)], 1).astype(np.float32)
    ref = (moved - np.float32([0.25, 0.0, 0.25]))[::-1].copy()
    return moved, np.full(8, 300, np.int32), np.arange(8)[::-1].astype(np.int32), ref, g


def test_the_split_limbs_hold_what_a_plain_64_bit_sum_wraps():
    moved, e, idx, ref, g = far_corner()
    assert TC.cells_numpy(moved, g)[0].all() and TC.cells_numpy(ref, g)[0].all()     # keyed: inside the grid
    a, b = S.bins_numpy(moved, g), S.bins_numpy(ref[idx], g)
    assert a.min() > (1 << 31) - 2048 and a.max() < 1 << 31 and b.min() > (1 << 31) - 2048 and b.max() < 1 << 31
    s = S.sums_numpy(moved, e, idx, ref, g)
    assert s == sums_of(a.tolist(), b.tolist(), e.tolist())
    exact = [[sum(int(x[r]) * int(y[c]) for x, y in zip(a, b)) for c in range(3)] for r in range(3)]
    M = [[(s[16 + 3 * r + c] << 32) + s[7 + 3 * r + c] for c in range(3)] for r in range(3)]
    assert M == exact and min(min(row) for row in exact) > 1 << 64
    # the same products in one 64-bit accumulator: every entry wraps (eight products just below 2^62 sum to just below 2^65)
    plain = (a[:, :, None] * b[:, None, :]).sum(0, dtype=np.int64)
    assert all(int(plain[r, c]) != exact[r][c] and int(plain[r, c]) == (exact[r][c] + (1 << 63)) % (1 << 64) - (1 << 63)
               for r in range(3) for c in range(3))
    dT, info = CR.solve(s, g)   # and the solve sees the shift: (-0.25, 0, -0.25)
    assert np.abs(dT[:3, 3] - [-0.25, 0.0, -0.25]).max() < 1e-6 and np.abs(dT[:3, :3] - np.eye(3)).max() < 1e-9


def test_both_routes_of_the_restated_sums_agree():
    p, q, _ = S.scene(True)
    g = cloud.CloudGrid(S.BORDER, 1.0)
    e, idx, _ = TCC.nearest_cells(p, q, g)
    small = S.sums_numpy(p, e, idx, q, g, 600)
    rep = 2   # 6000 pairs: past the Python-integer route
    big = S.sums_numpy(np.tile(p, (rep, 1)), np.tile(e, rep), np.tile(idx, rep), q, g, 600)
    assert big == [rep * v for v in small] and 0 < small[0] < len(p)
    # an idx outside the reference and an e above e_max are ignored; idx = -1 too
    e2, idx2 = e.copy(), idx.copy()
    idx2[:5], e2[5:9] = [len(q), len(q) + 7, -1, -5, 1 << 30], 601
    keep = np.ones(len(p), bool)
    keep[:9] = False
    assert S.sums_numpy(p, e2, idx2, q, g, 600) == S.sums_numpy(p[keep], e[keep], idx[keep], q, g, 600)


# ----------------------------------------------------------------------------------------
# the restatement on the scene
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [(1.0,), (1.0, 0.5)], ids=str)
def test_the_scene_with_the_same_points_on_both_sides(caps):
    T, log, moved = S.registered(False, caps)
    p, q, truth = S.scene(False)
    err = S.corner_error(T, truth)
    print("same points, caps %s: %d iterations, corner error %.3e (bound %.3e)" % (caps, len(log), err, SAME_POINTS_BOUND[caps]))
    assert S.corner_error(np.eye(4), truth) > 0.9                      # where it starts
    assert err < SAME_POINTS_BOUND[caps]
    ends = [e for e in log if "reason" in e]
    assert [e["reason"] for e in ends] == ["converged"] * len(caps) and [e["cap"] for e in ends] == list(caps) and len(log) < 20
    assert all(e["pairs"] == len(p) for e in log) and log[0]["rms"] > 0.25 and log[-1]["rms"] < 1e-3
    assert [e["iteration"] for e in log if e["stage"] == 1] == list(range(1, ends[0]["iteration"] + 1))
    assert np.abs(moved.astype(np.float64) - q).max() < 1e-4          # the same points, so they meet


@pytest.mark.parametrize("caps", [(1.0,), (1.0, 0.5)], ids=str)
def test_the_scene_with_a_separately_drawn_sample(caps):
    T, log, moved = S.registered(True, caps)
    truth = S.scene(True)[2]
    err = S.corner_error(T, truth)
    print("separate samples, caps %s: %d iterations, corner error %.3e (bound %.3e)" % (caps, len(log), err, SEPARATE_BOUND))
    assert err < SEPARATE_BOUND
    assert [e["reason"] for e in log if "reason" in e] == ["converged"] * len(caps) and log[-1]["rms"] < log[0]["rms"]


def test_max_iterations_init_and_a_degenerate_start():
    p, q, truth = S.scene(False)
    T1, log1, _ = S.register_numpy(p, q, S.BORDER, [1.0], max_iterations=1)
    full = S.registered(False, (1.0,))[1]
    assert len(log1) == 1 and log1[0]["reason"] == "iterations" and {k: v for k, v in log1[0].items() if k != "reason"} == full[0]
    T2, log2, _ = S.register_numpy(p, q, S.BORDER, [1.0], init=S.registered(False, (1.0,))[0])
    assert len(log2) == 1 and log2[0]["reason"] == "converged" and log2[0]["moved"] < 1.0 / 1024
    # a cloud out of the reference's reach: no pair, the stage ends at once and T stays what it was
    far = (p + np.float32([0, 0, 4.5])).astype(np.float32)
    T3, log3, moved3 = S.register_numpy(far, q, S.BORDER, [1.0, 0.5])
    assert np.array_equal(T3, np.eye(4)) and [e["reason"] for e in log3] == ["degenerate"] * 2 and [e["pairs"] for e in log3] == [0, 0]
    assert np.array_equal(moved3, far)
    # the pair cap: fewer pairs count, and a cap that is not a bin in 1 .. 1023 is refused
    T4, log4, _ = S.register_numpy(p, q, S.BORDER, [1.0], max_pair_dist=0.4, max_iterations=2)
    assert log4[0]["pairs"] < full[0]["pairs"]
    with pytest.raises(ValueError, match="1 .. 1023"):
        S.register_numpy(p, q, S.BORDER, [1.0], max_pair_dist=1.0)


def test_the_fscore_rises_from_below_a_half_to_above_nine_tenths():
    """The bounds tests/test_cloud_register_gpu.py holds the file tools to, checked here on the restatement first: the threshold is
    an eighth of the cap."""
    p, q, _ = S.scene(False)
    g = cloud.CloudGrid(S.BORDER, 1.0)
    score = lambda x: TCC.stats_numpy(TCC.nearest_cells(x, q, g)[2], TCC.nearest_cells(q, x, g)[2], 1.0, [0.125], (len(x), len(q)))["thresholds"][0]["fscore"]
    before, after = score(p), score(S.registered(False, (1.0,))[2])
    print("fscore at 0.125: %.4f unregistered, %.4f registered" % (before, after))
    assert before < 0.5 and after > 0.9


# ----------------------------------------------------------------------------------------
# order
# ----------------------------------------------------------------------------------------
def test_the_sums_do_not_depend_on_the_order_of_either_cloud_without_exact_ties():
    p, q, _ = S.scene(True)
    g = cloud.CloudGrid(S.BORDER, 1.0)
    e, idx, _ = TCC.nearest_cells(p, q, g)
    want = S.sums_numpy(p, e, idx, q, g)
    rng = np.random.default_rng(3)
    pp, pq = rng.permutation(len(p)), rng.permutation(len(q))
    e2, idx2, _ = TCC.nearest_cells(p[pp], q, g)
    assert np.array_equal(e2, e[pp]) and np.array_equal(idx2, idx[pp]) and S.sums_numpy(p[pp], e2, idx2, q, g) == want
    # the scene has no exact ties: the nearest reference POINT of every query is the same under a permutation of the reference
    e3, idx3, _ = TCC.nearest_cells(p, q[pq], g)
    assert np.array_equal(e3, e) and np.array_equal(q[pq][idx3[idx3 >= 0]], q[idx[idx >= 0]]) and S.sums_numpy(p, e3, idx3, q[pq], g) == want


def test_with_exact_ties_idx_and_the_sums_follow_the_order_of_the_reference():
    """Queries at the middle of a lattice's edges have two nearest reference points at the same distance and different positions;
    the nearest rule picks the lowest input index, so a reversed reference gives other idx, other b and other sums (N, sum a, sum e
    and sum e^2 stay).  The module's docstring says so."""
    g = TC.unit_grid(6, 6, 3)
    ax = np.arange(0.5, 5.5 + 1e-9, 0.25)
    q = np.stack(np.meshgrid(ax, ax, np.arange(0.5, 2.5 + 1e-9, 0.25), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = q[np.random.default_rng(6).permutation(len(q))]
    p = (q[:400].astype(np.float64) + [0.125, 0, 0]).astype(np.float32)
    e, idx, _ = TCC.nearest_numpy(p, q, g)
    r = q[::-1].copy()
    e2, idx2, _ = TCC.nearest_numpy(p, r, g)
    assert np.array_equal(e, e2) and (e == 128).all() and (idx >= 0).all()
    assert (q[idx] != r[idx2]).any(1).mean() > 0.9                      # another point of the pair, for most queries
    s, s2 = S.sums_numpy(p, e, idx, q, g), S.sums_numpy(p, e2, idx2, r, g)
    same = [0, 1, 2, 3, 25, 26]
    assert [s[k] for k in same] == [s2[k] for k in same] and s[4] != s2[4] and s[7:25] != s2[7:25]


# ----------------------------------------------------------------------------------------
# files and command lines
# ----------------------------------------------------------------------------------------
def test_the_transform_file_round_trips_exactly(tmp_path):
    T = S.registered(True, (1.0,))[0]
    path = CR.write_transform(tmp_path / "sub" / "T.txt", T)
    text = open(path).read()
    assert len(text.strip().split("\n")) == 4 and all(len(ln.split()) == 4 for ln in text.strip().split("\n"))
    back = CR.read_transform(path)
    assert back.dtype == np.float64 and back.tobytes() == np.ascontiguousarray(T).tobytes()
    odd = np.eye(4)
    odd[:3] = [[1e-300, -0.0, 1 / 3, 5e-324], [2.0 ** 60 + 1, -1e300, math.pi, 0.1], [1, 2, 3, 4]]
    assert CR.read_transform(CR.write_transform(tmp_path / "odd.txt", odd)).tobytes() == odd.tobytes()
    for name, body, msg in (("three.txt", "1 0 0 0\n0 1 0 0\n0 0 1 0\n", "four lines"), ("five.txt", "1 0 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n", "four lines"),
                            ("word.txt", "1 0 0 0\n0 x 0 0\n0 0 1 0\n0 0 0 1\n", "four lines"), ("row.txt", "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 2\n", "0 0 0 1"),
                            ("nan.txt", "1 0 0 nan\n0 1 0 0\n0 0 1 0\n0 0 0 1\n", "finite"), ("inf.txt", "1 0 0 0\n0 inf 0 0\n0 0 1 0\n0 0 0 1\n", "finite")):
        (tmp_path / name).write_text(body)
        with pytest.raises(ValueError, match=msg):
            CR.read_transform(tmp_path / name)
    for bad, msg in ((np.eye(3), "4 x 4"), (np.full((4, 4), np.nan), "finite"), (np.ones((4, 4)), "0 0 0 1"), ("T", "4 x 4")):
        with pytest.raises(ValueError, match=msg):
            CR.write_transform(tmp_path / "bad.txt", bad)
    assert not (tmp_path / "bad.txt").exists()


def test_xyz_ply_bytes_are_read_back_by_read_xyz_ply(tmp_path):
    xyz = S.scene(False)[0][:37]
    (tmp_path / "a.ply").write_bytes(CR.xyz_ply_bytes(xyz))
    assert np.array_equal(CC.read_xyz_ply(tmp_path / "a.ply"), xyz)
    assert CR.xyz_ply_bytes(torch.from_numpy(xyz)) == CR.xyz_ply_bytes(xyz)
    (tmp_path / "none.ply").write_bytes(CR.xyz_ply_bytes(np.zeros((0, 3), np.float32)))
    assert CC.read_xyz_ply(tmp_path / "none.ply").shape == (0, 3)
    with pytest.raises(ValueError, match="float32"):
        CR.xyz_ply_bytes(xyz.astype(np.float64))


def test_the_command_line_refuses_before_it_reads_or_writes(capsys, tmp_path):
    a, b, t0 = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "t0.txt")   # none of them exists
    out = tmp_path / "out"
    base = ["--cloud", a, "--reference", b, "--border=0,8,0,4,-1,1", "--max_dist=0.5,0.25"]
    outs = ["--out_transform", str(out / "T.txt"), "--out", str(out / "r.ply"), "--json", str(out / "r.json")]
    cases = [base[2:] + outs, base[:2] + base[4:] + outs, base[:4] + base[5:] + outs, base[:5] + outs,
             base[:4] + ["--border=0,8,0,4"] + base[5:], base[:5] + ["--max_dist=0.25,0.5"], base[:5] + ["--max_dist=0.5,0.5"],
             base[:5] + ["--max_dist=0.5,x"], base[:5] + ["--max_dist=0"], base[:5] + ["--max_dist=1e-9"],
             base + ["--iterations=0"], base + ["--tolerance=0"], base + ["--tolerance=nan"], base + ["--max_pair_dist=0.25"],
             base + ["--max_pair_dist=0.00001"], base + ["--init", str(tmp_path / "t0.json")], base + ["--out_transform", str(out / "T.json")],
             base + ["--out", str(out / "r.xyz")], base + ["--json", str(out / "r.txt")],
             base + ["--out_transform", str(out / "T.txt"), "--init", str(out / "T.txt")], base + ["--out", a],
             base + ["--out", str(out / "r.ply"), "--json", str(out / "r.ply")]]
    for argv in cases:
        with pytest.raises(SystemExit):
            CR.main(argv)
    err = capsys.readouterr().err
    for text in ("--cloud is required", "--reference is required", "--border is required", "--max_dist is required", "got 4 values", "decrease strictly",
                 "H1[,H2...]", "max_dist must be finite", "2^21", "max_iterations", "tolerance must be finite", "1 .. 1023", "--init must end in .txt",
                 "--out_transform must end in .txt", "--out must end in .ply", "--json must end in .json", "overwrite an input"):
        assert text in err, text
    assert not out.exists()
    # a well-formed command line gets as far as the GPU or the first missing file
    with pytest.raises((RuntimeError, OSError)):
        CR.main(base + ["--init", t0] + outs)
    assert not out.exists()


def test_the_compare_tools_refuse_a_bad_transform_flag_before_they_read_or_write(capsys, tmp_path):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    out = tmp_path / "out"
    cloud_argv = ["--cloud", a, "--reference", b, "--border=0,8,0,4,-1,1", "--max_dist=0.5", "--threshold=0.1", "--json", str(out / "T.txt.json")]
    mesh_argv = ["--mesh", a, "--reference", b, "--border=0,8,0,4,-1,1", "--max_dist=0.5", "--threshold=0.1", "--spacing=0.1", "--out_mesh", str(out / "m.ply")]
    for main, argv, own in ((CC.main, cloud_argv, str(out / "T.txt.json")), (MC.main, mesh_argv, str(out / "m.ply"))):
        for bad in (str(tmp_path / "T.json"), own, a, b):
            with pytest.raises(SystemExit):
                main(argv + ["--transform", bad])
        with pytest.raises(SystemExit):
            main(argv + ["--transform"])
        err = capsys.readouterr().err
        for text in ("--transform must end in .txt", "expected one argument"):
            assert text in err, text
        # with the flag well-formed the tool goes on as without it: to the GPU, or to the first missing file
        with pytest.raises((RuntimeError, OSError)):
            main(argv + ["--transform", str(tmp_path / "T.txt")])
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
    assert len(_lib.SIGNATURES["d3d_cloud_transform"]) == 5 and len(_lib.SIGNATURES["d3d_cloud_register_sums"]) == 13
    L, D, I, V = ctypes.c_longlong, ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["d3d_cloud_transform"] == [V, L, V, V, V]
    assert _lib.SIGNATURES["d3d_cloud_register_sums"] == [V, V, V, L, V, L, D, D, D, D, I, V, V]
    _lib.build()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, s) for s in NEW_SYMBOLS)
    assert _lib.load().d3d_build_flags() == b""


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)   # fake pointers 4 GiB apart, never dereferenced: every call below fails its checks first
    n = 10
    order = ["xyz", "n", "rt", "out", "st"]
    ok = dict(xyz=P(1), n=n, rt=P(2), out=P(3), st=None)
    size = dict(xyz=12 * n, rt=96, out=12 * n)
    alias = []
    for a, b in itertools.combinations(size, 2):   # the second begins on the last byte of the first, and the other way round
        alias.append((dict([(b, ctypes.c_void_p(ok[a].value + size[a] - 1))]), b"alias"))
        alias.append((dict([(a, ctypes.c_void_p(ok[b].value + size[b] - 1))]), b"alias"))
    assert len(alias) == 6
    TC._expect(lib, lib.d3d_cloud_transform, ok, order,
               [(dict([(name, None)]), b"null") for name in size] + [(dict(n=-1), b"n="), (dict(n=1 << 31), b"n=")] + alias)
    assert lib.d3d_cloud_transform(None, 0, None, None, None) == 0   # no point: nothing to do, nothing launched

    nq, nt = 10, 7
    order = ["qx", "e", "idx", "nq", "tx", "nt", "x0", "y0", "z0", "h", "emax", "sums", "st"]
    ok = dict(qx=P(1), e=P(2), idx=P(3), nq=nq, tx=P(4), nt=nt, x0=-1.0, y0=2.0, z0=0.0, h=0.5, emax=1024, sums=P(5), st=None)
    size = dict(qx=12 * nq, e=4 * nq, idx=4 * nq, tx=12 * nt, sums=8 * 27)
    alias = []
    for a, b in itertools.combinations(size, 2):
        alias.append((dict([(b, ctypes.c_void_p(ok[a].value + size[a] - 1))]), b"alias"))
        alias.append((dict([(a, ctypes.c_void_p(ok[b].value + size[b] - 1))]), b"alias"))
    assert len(alias) == 20
    TC._expect(lib, lib.d3d_cloud_register_sums, ok, order,
               [(dict([(name, None)]), b"null") for name in size] +
               [(dict(nq=-1), b"n_query"), (dict(nq=1 << 31), b"n_query"), (dict(nt=-1), b"n_target"), (dict(nt=1 << 31), b"n_target"),
                (dict(x0=math.nan), b"origin"), (dict(y0=math.inf), b"origin"), (dict(z0=-math.inf), b"origin"),
                (dict(h=0.0), b"cap"), (dict(h=-1.0), b"cap"), (dict(h=math.nan), b"cap"), (dict(h=math.inf), b"cap"),
                (dict(emax=-1), b"e_max"), (dict(emax=1025), b"e_max"),
                # no query, no target: the sums are still needed
                (dict(nq=0, qx=None, e=None, idx=None, sums=None), b"null"), (dict(nt=0, tx=None, sums=None), b"null")] + alias)


def test_the_operator_refuses_cpu_tensors_bad_dtypes_shapes_and_settings():
    g = TC.unit_grid()
    xyz, e, idx = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.apply(xyz, np.eye(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.pair_sums(xyz, e, idx, xyz.clone(), g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CR.register(xyz, xyz.clone(), g.border, [1.0])
    for bad in (xyz.double(), torch.zeros(5, 2), torch.zeros(15), torch.zeros(5, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="xyz"):
            CR.apply(bad, np.eye(4))
        with pytest.raises(ValueError, match="moved_xyz"):
            CR.pair_sums(bad, e, idx, xyz, g)
        with pytest.raises(ValueError, match="reference_xyz"):
            CR.pair_sums(xyz, e, idx, bad, g)
        with pytest.raises(ValueError, match="cloud_xyz"):
            CR.register(bad, xyz, g.border, [1.0])
    with pytest.raises(TypeError, match="Tensor"):
        CR.apply(np.zeros((5, 3), np.float32), np.eye(4))
    for T, msg in ((np.eye(3), "4 x 4"), (np.full((4, 4), np.inf), "finite"), (2 * np.eye(4), "0 0 0 1"), (None, "4 x 4")):
        with pytest.raises(ValueError, match=msg):
            CR.apply(xyz, T)
    with pytest.raises(ValueError, match="init"):
        CR.register(xyz, xyz, g.border, [1.0], init=2 * np.eye(4))
    for be, bi, msg in ((e.long(), idx, "e must"), (e, idx[:4], "idx must"), (e.float(), idx, "e must")):
        with pytest.raises(ValueError, match=msg):
            CR.pair_sums(xyz, be, bi, xyz, g)
    with pytest.raises(TypeError, match="Tensor"):
        CR.pair_sums(xyz, e.numpy(), idx, xyz, g)
    with pytest.raises(TypeError, match="CloudGrid"):
        CR.pair_sums(xyz, e, idx, xyz, g.border)
    for bad in (-1, 1025, 0.5, True):
        with pytest.raises(ValueError, match="e_max"):
            CR.pair_sums(xyz, e, idx, xyz, g, bad)
    for kw, msg in ((dict(max_dists=[0.5, 1.0]), "decrease strictly"), (dict(max_dists=[1.0, 1.0]), "decrease strictly"), (dict(max_dists=[]), "at least one"),
                    (dict(max_dists=[0.0]), "max_dist"), (dict(max_dists=[1e-9]), "2\\^21"), (dict(border=[0, 4, 0, 4]), "six"),
                    (dict(max_iterations=0), "max_iterations"), (dict(max_iterations=2.5), "max_iterations"), (dict(tolerance=0.0), "tolerance"),
                    (dict(tolerance=math.inf), "tolerance"), (dict(max_pair_dist=1.0), "1 .. 1023"), (dict(max_pair_dist=0.6, max_dists=[1.0, 0.5]), "1 .. 1023")):
        with pytest.raises(ValueError, match=msg):
            CR.register(**dict(dict(cloud_xyz=xyz, reference_xyz=xyz, border=g.border, max_dists=[1.0]), **kw))


def test_the_kernels_use_integer_atomic_add_only_and_the_build_lists_the_source():
    strip = lambda s: re.sub(r"//[^\n]*|/\*.*?\*/", "", s, flags=re.S)
    hip = strip(open(_lib.CSRC + "/cloud_register.hip").read())
    assert set(re.findall(r"\batomic\w*", hip)) == {"atomicAdd"}
    assert not re.search(r"unsafeAtomic|atomicAdd\s*\(\s*\(?\s*(float|double)\s*\*|__hip_atomic|__builtin_amdgcn_\w*atomic", hip)
    # the one atomicAdd is a statement (its result is not used), on the unsigned 64-bit sums in memory
    assert len(re.findall(r"(?:^|[;{}\)])\s*atomicAdd\(", hip, re.M)) == len(re.findall(r"\batomicAdd\(", hip)) == 1
    assert "atomicAdd(sums + tid, (unsigned long long)v)" in hip and re.search(r"unsigned long long\* __restrict__ sums\)", hip)
    assert "fma" not in hip and "asm" not in hip
    # the shared helpers are included, not restated
    assert '#include "cloud_search.h"' in hip and '#include "geom_shared.h"' in hip and "search_apart(" in hip and "wave_sum(" in hip
    assert "search_resident(" in hip and "struct SearchRange" not in hip and "inline bool search_apart" not in hip and "__shfl" not in hip
    assert "hipOccupancy" not in hip and "hipOccupancy" not in strip(open(_lib.CSRC + "/cloud_compare.hip").read())
    make = open(_lib.CSRC + "/Makefile").read()
    assert re.search(r"^SRCS :=.*\bcloud_register\.hip\b", make, re.M) and re.search(r"^HDRS :=.*\bcloud_search\.h\b", make, re.M)
    assert "-ffp-contract=off" in make
    # the module allocates nothing numpy leaves unwritten (tests/test_poison.py keeps an exact list of those)
    assert "np.empty" not in open(CR.__file__).read()
