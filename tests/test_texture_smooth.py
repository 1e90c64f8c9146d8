"""Smoothing the texture's view choice on the CPU: a numpy restatement of the rule in deep3d_aerial_amd/texture.py (candidate
lists and rounds; tests/test_texture_smooth_gpu.py compares the kernels with it bit for bit), its invariants on the rough grid,
hand-built cases, and the plumbing: entry points, settings and command-line flags."""
import os
import re

import numpy as np
import pytest

import test_texture as T

EMPTY = T.EMPTY
K = 16


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def candidates_numpy(vertices, faces, views, depth_tolerance=0.01):
    """cand [m, 16] int64: per face the 16 smallest keys over the views that accept it, increasing, padded with INT64_MAX."""
    m = len(faces)
    per_view = [T.select_numpy(vertices, faces, [v], depth_tolerance) for v in views]   # one view: its key, or EMPTY
    allk = np.stack(per_view + [np.full(m, EMPTY, np.int64)] * K, 1)
    return np.ascontiguousarray(np.sort(allk, 1)[:, :K])


def merge_numpy(a, b):
    out = np.full(a.shape, EMPTY, np.int64)
    for f in range(a.shape[0]):
        u = np.unique(np.concatenate([a[f], b[f]]))
        u = u[u != EMPTY][:K]
        out[f, :len(u)] = u
    return out


def winners(faces, cand):
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    distinct = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])
    return distinct & (cand[:, 0] != EMPTY)


def neighbour_pairs(faces, has):
    """(f, g, w) over the ordered pairs of distinct faces with winners that share w >= 1 vertices."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    by_vertex = {}
    for f in np.flatnonzero(has):
        for v in F[f]:
            by_vertex.setdefault(int(v), []).append(int(f))
    count = {}
    for fs in by_vertex.values():
        for f in fs:
            for g in fs:
                if f != g:
                    count[(f, g)] = count.get((f, g), 0) + 1
    if not count:
        z = np.zeros(0, np.int64)
        return z, z, z
    fg = np.array(sorted(count), np.int64)
    return fg[:, 0], fg[:, 1], np.array([count[tuple(p)] for p in fg], np.int64)


def data_terms(cand):
    """d [m, 16] fp32 = 1 - s_0 / s_k (rows without a key: whatever; they are never read)."""
    s = (cand >> 32).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(1.0) - s[:, :1] / s).astype(np.float32)


def ids_of(cand):
    return (cand & 0xffffffff).astype(np.int64)


def energy(cand, label, has, pairs, weight):
    """E in fp64."""
    s = (cand >> 32).astype(np.uint32).view(np.float32).astype(np.float64)
    fs = np.flatnonzero(has)
    E = float((1.0 - s[fs, 0] / s[fs, label[fs]]).sum())
    pf, pg, pw = pairs
    cur = ids_of(cand)[np.arange(len(cand)), np.maximum(label, 0)]
    half = pf < pg
    return E + float(weight) * float((pw[half] * (cur[pf[half]] != cur[pg[half]])).sum())


def smooth_rounds_numpy(faces, cand, weight, max_loss=0.25, rounds=64):
    """Yields (label [m] int32, committed [m] bool) after each round, the first round without a commit included."""
    cand = np.asarray(cand, np.int64)
    m = cand.shape[0]
    has = winners(faces, cand)
    pf, pg, pw = neighbour_pairs(faces, has)
    d, ids = data_terms(cand), ids_of(cand)
    ok = (cand != EMPTY) & (d <= np.float32(max_loss))
    ok[:, 0] = True
    lam = np.float32(weight)
    label = np.where(has, 0, -1).astype(np.int32)
    rows = np.arange(m)
    for _ in range(rounds):
        cur = ids[rows, np.maximum(label, 0)]
        n = np.zeros((m, K), np.int64)
        np.add.at(n, pf, pw[:, None] * (cur[pg][:, None] != ids[pf]))
        c = (d + (lam * n.astype(np.float32)).astype(np.float32)).astype(np.float32)
        best = np.argmin(np.where(ok, c, np.float32(np.inf)), 1)   # the first of equal costs: the smallest k
        gain = (c[rows, np.maximum(label, 0)] - c[rows, best]).astype(np.float32)
        want = has & (gain > 0)
        prio = np.where(want, (gain.view(np.uint32).astype(np.int64) << 32) | ((1 << 32) - 1 - rows), 0)
        top = np.zeros(m, np.int64)
        np.maximum.at(top, pf, prio[pg])
        take = want & (prio > top)
        label = np.where(take, best, label).astype(np.int32)
        yield label, take
        if not take.any():
            return


def smooth_numpy(faces, cand, weight, max_loss=0.25, rounds=64):
    """(key [m] int64, label [m] int32, commits: each round's number of changes, cut at the first round without one)."""
    cand = np.asarray(cand, np.int64)
    label = np.where(winners(faces, cand), 0, -1).astype(np.int32)
    commits = []
    for label, take in smooth_rounds_numpy(faces, cand, weight, max_loss, rounds):
        if not take.any():
            break
        commits.append(int(take.sum()))
    key = np.where(label >= 0, cand[np.arange(len(cand)), np.maximum(label, 0)], EMPTY)
    return key, label, np.array(commits, np.int32)


# ----------------------------------------------------------------------------------------
# the rough grid
# ----------------------------------------------------------------------------------------
def rough_grid(N, seed=0):
    """(vertices [(N+1)^2, 3] fp32, faces [2 N^2, 3] int32, cand [2 N^2, 16]): integer x, y, z = normal(0, 0.03); two triangles per
    cell; 16 pinhole cameras (f = 40) looking straight down from height 12 on a 4 x 4 grid over [0, N]^2, every one of them a
    candidate of every face, the keys from the projected areas."""
    z = np.random.default_rng(seed).normal(0.0, 0.03, (N + 1) * (N + 1))
    ys, xs = np.mgrid[0:N + 1, 0:N + 1]
    V = np.stack([xs.ravel(), ys.ravel(), z], 1).astype(np.float32)
    F = []
    for i in range(N):
        for j in range(N):
            a, b, c, d = i * (N + 1) + j, i * (N + 1) + j + 1, (i + 1) * (N + 1) + j, (i + 1) * (N + 1) + j + 1
            F += [[a, b, c], [b, d, c]]
    F = np.array(F, np.int32)
    P = V.astype(np.float64)[F]   # [m, 3 corners, 3]
    keys = []
    for k in range(16):
        cx, cy = N * (k % 4 + 0.5) / 4, N * (k // 4 + 0.5) / 4
        depth = 12.0 - P[:, :, 2]
        u, v = 40.0 * (P[:, :, 0] - cx) / depth, 40.0 * (P[:, :, 1] - cy) / depth
        A = 0.5 * np.abs((u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (u[:, 2] - u[:, 0]) * (v[:, 1] - v[:, 0]))
        keys.append(T.make_key(1.0 / A, k))
    return V, F, np.ascontiguousarray(np.sort(np.stack(keys, 1), 1))


def n_charts(faces, key):
    return len(T.charts_numpy(faces, key)[1])


@pytest.mark.parametrize("max_loss", [0.25, 1.0])
def test_every_round_keeps_the_invariants_on_the_rough_grid(max_loss):
    _, F, cand = rough_grid(12)
    has = winners(F, cand)
    pairs = neighbour_pairs(F, has)
    pf, pg, _ = pairs
    d = data_terms(cand)
    label = np.zeros(len(F), np.int32)
    E = energy(cand, label, has, pairs, 0.1)
    n_rounds = 0
    for label, take in smooth_rounds_numpy(F, cand, 0.1, max_loss, 256):
        assert not (take[pf] & take[pg]).any()   # no two neighbouring faces commit
        E1 = energy(cand, label, has, pairs, 0.1)
        assert E1 <= E + 1e-5
        E = E1
        assert (d[np.arange(len(F)), label] <= np.float32(max_loss)).all()
        n_rounds += 1
    assert not take.any() and 3 < n_rounds < 256   # it reached the fixed point


def test_a_vanishing_weight_changes_nothing():
    _, F, cand = rough_grid(12)
    key, label, commits = smooth_numpy(F, cand, 1e-30)
    assert (label == 0).all() and len(commits) == 0 and np.array_equal(key, cand[:, 0])


def test_smoothing_leaves_at_most_half_the_charts_within_64_rounds():
    _, F, cand = rough_grid(24)
    before = n_charts(F, cand[:, 0])
    states = list(smooth_rounds_numpy(F, cand, 0.1, 0.25, 64))
    assert not states[-1][1].any(), "no fixed point within 64 rounds"
    key, label, commits = smooth_numpy(F, cand, 0.1, 0.25, 64)
    after = n_charts(F, key)
    print("rough 24 x 24 grid: %d charts -> %d in %d rounds" % (before, after, len(commits)))
    assert np.array_equal(label, states[-1][0]) and len(commits) == len(states) - 1
    assert before > 100 and 2 * after <= before


# ----------------------------------------------------------------------------------------
# hand-built cases
# ----------------------------------------------------------------------------------------
def row(*pairs):
    r = np.full(K, EMPTY, np.int64)
    for i, (s, vid) in enumerate(pairs):
        r[i] = T.make_key(s, vid)
    return r


def test_of_two_neighbours_with_bit_equal_gains_the_lower_index_commits():
    F = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    cand = np.stack([row((1.0, 1), (1.1, 2)), row((1.0, 2), (1.1, 1))])
    states = list(smooth_rounds_numpy(F, cand, 0.1))
    assert list(states[0][0]) == [1, 0] and list(states[0][1]) == [True, False]
    assert len(states) == 2 and not states[1][1].any()   # face 1 now agrees with face 0: nothing left to gain
    key, label, commits = smooth_numpy(F, cand, 0.1)
    assert list(label) == [1, 0] and list(commits) == [1] and list(key & 0xffffffff) == [2, 2]
    # with the faces swapped it is again the lower index
    _, label, _ = smooth_numpy(F[::-1], cand[::-1], 0.1)
    assert list(label) == [1, 0]


def test_a_face_whose_only_agreeing_view_is_inadmissible_stays():
    F = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    cand = np.stack([row((1.0, 1), (2.0, 2)), row((1.0, 2))])   # d = 0.5 > 0.25
    key, label, commits = smooth_numpy(F, cand, 0.1, 0.25)
    assert list(label) == [0, 0] and len(commits) == 0
    _, label, commits = smooth_numpy(F, cand, 0.4, 0.5)   # admissible, and 2 * 0.4 > 0.5
    assert list(label) == [1, 0] and list(commits) == [1]


def test_a_face_without_a_winner_is_never_counted_and_never_labelled():
    V, F = T.strip(2)   # faces 0 1 2 3; 1 shares an edge with 0 and with 2
    cand = np.stack([row((1.0, 1), (1.05, 2)), row(), row((1.0, 2), (1.05, 1)), row((1.0, 2))])
    has = winners(F, cand)
    pf, pg, pw = neighbour_pairs(F, has)
    assert list(has) == [True, False, True, True] and 1 not in pf and 1 not in pg
    assert {(int(a), int(b)): int(w) for a, b, w in zip(pf, pg, pw)} == {(0, 2): 1, (2, 0): 1, (2, 3): 2, (3, 2): 2}
    key, label, commits = smooth_numpy(F, cand, 0.1)
    assert label[1] == -1 and key[1] == EMPTY
    assert list(label) == [1, -1, 0, 0] and list(commits) == [1]   # face 0 joins view 2 across the vertex it shares with face 2
    # a face with a repeated index has no winner either, whatever its row holds
    F2 = F.copy()
    F2[2] = [F[2][0], F[2][0], F[2][1]]
    _, label, commits = smooth_numpy(F2, cand, 0.1)
    assert list(label) == [0, -1, -1, 0] and len(commits) == 0


def test_candidates_keep_the_sixteen_smallest_and_merge_by_halves():
    rng = np.random.default_rng(3)
    V, F = T.strip(3)
    views = [T.cam_view(100 + i, C=(rng.uniform(0, 3), rng.uniform(0, 1), 0.0), f=float(rng.uniform(20, 50))) for i in range(20)]
    cand = candidates_numpy(V, F, views)
    assert (cand[:, -1] != EMPTY).all()   # every face passes more than 16 views here
    assert (np.diff(cand, axis=1) > 0).all()
    assert np.array_equal(cand[:, 0], T.select_numpy(V, F, views))
    assert np.array_equal(merge_numpy(candidates_numpy(V, F, views[:7]), candidates_numpy(V, F, views[7:])), cand)
    assert np.array_equal(candidates_numpy(V, F, views[::-1]), cand)


# ----------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------
NAMES = ["d3d_texture_candidates_max", "d3d_texture_candidates", "d3d_texture_candidates_merge", "d3d_texture_smooth_scratch_bytes",
         "d3d_texture_smooth"]


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib, texture

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in _lib.SIGNATURES, n
    assert "texture_smooth.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    shared = open(os.path.join(_lib.CSRC, "texture_shared.h")).read()
    assert re.search(r"TX_CANDIDATES = %d\b" % texture.CANDIDATES, shared) and texture.CANDIDATES == K
    # the selection and the candidate lists run one statement of the per-view tests
    for src in ("texture.hip", "texture_smooth.hip"):
        assert "tx_view_key(" in open(os.path.join(_lib.CSRC, src)).read(), src


def test_the_library_refuses_bad_arguments():
    import ctypes

    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    assert lib.d3d_texture_candidates_max() == K
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before a launch
    run = ctypes.c_int(0)
    big = 1 << 40
    assert lib.d3d_texture_candidates(None, 4, None, 4, None, 0, 0.01, None, 0, None, None) == -1
    assert lib.d3d_texture_candidates(p, 4, p, 4, p, 3, -1.0, p, big, p, None) == -1
    assert lib.d3d_texture_candidates(p, 4, p, 4, p, 3, 0.01, p, 0, p, None) == -1 and b"scratch" in lib.d3d_last_error()
    assert lib.d3d_texture_candidates_merge(None, p, 4, p, None) == -1
    assert lib.d3d_texture_smooth_scratch_bytes(-1) == 0 and lib.d3d_texture_smooth_scratch_bytes(1 << 29) == 0   # 6 m >= 2^31
    assert lib.d3d_texture_smooth_scratch_bytes(10) >= 160
    good = lambda **kw: lib.d3d_texture_smooth(p, kw.get("m", 4), p, 4, p, p, kw.get("w", 0.1), kw.get("loss", 0.25), kw.get("rounds", 8), p,
                                               kw.get("bytes", big), p, p, p, ctypes.byref(run), None)
    for bad in ({"w": 0.0}, {"w": -1.0}, {"w": float("nan")}, {"loss": -0.1}, {"loss": 1.5}, {"rounds": 0}, {"rounds": 1025}, {"bytes": 16}):
        assert good(**bad) == -1, bad
    assert good(m=1 << 29) == -1 and b"6 n_faces" in lib.d3d_last_error()   # larger than the vertex -> face lists allow


def test_settings_and_argument_errors():
    from deep3d_aerial_amd import texture

    assert texture.check_smooth_settings({"weight": 0.1}) == (0.1, 0.25, 64)
    assert texture.check_smooth_settings({"weight": 2, "max_loss": 1, "rounds": 1024}) == (2.0, 1.0, 1024)
    for bad in ({}, {"weight": 0}, {"weight": -0.1}, {"weight": float("inf")}, {"weight": 0.1, "max_loss": -0.01},
                {"weight": 0.1, "max_loss": 1.01}, {"weight": 0.1, "rounds": 0}, {"weight": 0.1, "rounds": 1025},
                {"weight": 0.1, "rounds": 2.5}, {"weight": 0.1, "round": 3}):
        with pytest.raises(ValueError):
            texture.check_smooth_settings(bad)
    base = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in (["--smooth_views", "0"], ["--smooth_views", "-1"], ["--smooth_max_loss", "2"], ["--smooth_rounds", "0"],
                ["--smooth_views", "0.1", "--smooth_rounds", "2000"]):
        with pytest.raises(SystemExit):
            texture.main(base + bad)
    import torch

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.smooth_views(torch.zeros((2, 3), dtype=torch.int32), 4, torch.zeros((2, K), dtype=torch.int64), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.merge_candidates(torch.zeros((2, K), dtype=torch.int64), torch.zeros((2, K), dtype=torch.int64))


def test_the_flags_parse_with_and_without_the_prefix():
    import argparse

    from deep3d_aerial_amd import predict, texture

    ap = argparse.ArgumentParser()
    texture.add_arguments(ap)
    assert texture.settings_from_args(ap.parse_args([]), "o.ply")["smooth_views"] is None
    a = ap.parse_args(["--smooth_views", "0.1"])
    assert texture.settings_from_args(a, "o.ply")["smooth_views"] == {"weight": 0.1, "max_loss": 0.25, "rounds": 64}
    a = ap.parse_args(["--smooth_views", "0.3", "--smooth_max_loss", "0.5", "--smooth_rounds", "7"])
    assert texture.settings_from_args(a, "o.ply")["smooth_views"] == {"weight": 0.3, "max_loss": 0.5, "rounds": 7}
    base = ["--output_folder", "out", "--synthetic_items", "2", "--random_weights", "--fuse", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1",
            "--mesh_voxel=0.5", "--texture", "t.ply"]
    assert predict._texture_settings(predict.parse_args(base))["smooth_views"] is None
    a = predict.parse_args(base + ["--texture_smooth_views", "0.1", "--texture_smooth_rounds", "32"])
    assert predict._texture_settings(a)["smooth_views"] == {"weight": 0.1, "max_loss": 0.25, "rounds": 32}
    for bad in (["--texture_smooth_views", "0"], ["--texture_smooth_max_loss", "-1"]):
        with pytest.raises(SystemExit):
            predict.parse_args(base + bad)
