"""Rejecting outlier views from the texture's candidate lists on the CPU: a numpy restatement of the rule in
deep3d_aerial_amd/texture.py (the colour of a face in a candidate view and the vote; tests/test_texture_outliers_gpu.py compares
the kernels with it bit for bit), hand-built rows, the behaviour scene's numbers, and the plumbing: entry points, settings and
command-line flags."""
import os
import re

import numpy as np
import pytest

import test_texture as T
import test_texture_smooth as S

EMPTY = T.EMPTY
K = S.K
QMAX = 1020


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def tap_numpy(image, u, v):
    """ortho's bilinear tap of image [H, W, >= 3] uint8 at (u, v) [n] fp64, not rounded: [n, 3] fp64."""
    H, W = image.shape[:2]
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = u - fu, v - fv
    x0 = np.clip(fu, 0, W - 1).astype(np.int64)
    y0 = np.clip(fv, 0, H - 1).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    c = lambda y, x: image[y, x, :3].astype(np.float64)
    return ((w00[:, None] * c(y0, x0) + w10[:, None] * c(y0, x1)) + w01[:, None] * c(y1, x0)) + w11[:, None] * c(y1, x1)


def color_word(q):
    """2^30 | qR << 20 | qG << 10 | qB of q [..., 3] in quarter grey levels."""
    q = np.asarray(q, np.int64)
    return ((1 << 30) | (q[..., 0] << 20) | (q[..., 1] << 10) | q[..., 2]).astype(np.int32)


def colors_numpy(vertices, faces, cand, views, col=None):
    """col [m, 16] int32: the colour word of every slot of cand whose view is among `views`; other slots are left as they are
    (0 in a new col)."""
    cand = np.asarray(cand, np.int64)
    m = cand.shape[0]
    col = np.zeros((m, K), np.int32) if col is None else col.copy()
    a, b, c = T.corners(vertices, faces)
    for view in views:
        f, k = np.nonzero((cand != EMPTY) & ((cand & 0xffffffff) == view["id"]))
        if not len(f):
            continue
        ok = np.ones(len(f), bool)
        us, vs = [], []
        for X in (a[f], b[f], c[f]):
            p2, q2, u, v = T.project(view, X)
            with np.errstate(invalid="ignore"):
                ok &= (p2 > 0) & (q2 > 0) & np.isfinite(u) & np.isfinite(v)
            us.append(u)
            vs.append(v)
        f, k = f[ok], k[ok]
        u, v = [x[ok] for x in us], [x[ok] for x in vs]
        mix = lambda p: [((p[0] + p[1]) + p[2]) / 3.0, ((4.0 * p[0] + p[1]) + p[2]) / 6.0, ((4.0 * p[1] + p[0]) + p[2]) / 6.0,
                         ((4.0 * p[2] + p[0]) + p[1]) / 6.0]
        t = [tap_numpy(view["image"], su, sv) for su, sv in zip(mix(u), mix(v))]
        q = np.clip(np.floor((((t[0] + t[1]) + t[2]) + t[3]) + 0.5), 0, QMAX)
        col[f, k] = color_word(q)
    return col


def channels(col):
    """q [..., 3] of colour words."""
    col = np.asarray(col, np.int64)
    return np.stack([(col >> 20) & 1023, (col >> 10) & 1023, col & 1023], -1)


def deviations(cand, col):
    """(valid [m, 16], n [m], dev [m, 16] -- max over the channels of |q - lower median|, 0 on invalid slots)."""
    cand, col = np.asarray(cand, np.int64), np.asarray(col, np.int32)
    valid = (cand != EMPTY) & (col != 0)
    n = valid.sum(1)
    q = channels(col)
    dev = np.zeros(cand.shape, np.int64)
    for f in np.flatnonzero(n > 0):
        vals = q[f][valid[f]]   # [n, 3]
        med = np.sort(vals, 0)[(n[f] - 1) >> 1]
        dev[f, valid[f]] = np.abs(vals - med).max(1)
    return valid, n, dev


def reject_numpy(cand, col, threshold):
    """(cand_out [m, 16], rejected [m] int32, counts [4]: faces tested, column 0 changed, slots removed, kept_all faces)."""
    cand = np.asarray(cand, np.int64)
    T_ = int(np.floor(float(threshold) * QMAX))
    valid, n, dev = deviations(cand, col)
    out = valid & (dev > T_) & (n >= 3)[:, None]
    kept_all = (n >= 3) & (out.sum(1) == n)
    out[kept_all] = False
    keep = (cand != EMPTY) & ~out
    cand_out = np.full(cand.shape, EMPTY, np.int64)
    for f in range(cand.shape[0]):
        ks = cand[f][keep[f]]
        cand_out[f, :len(ks)] = ks
    rejected = (out.astype(np.int64) << np.arange(K)).sum(1).astype(np.int32)
    counts = np.array([(n >= 3).sum(), (cand_out[:, 0] != cand[:, 0]).sum(), out.sum(), kept_all.sum()], np.int32)
    return cand_out, rejected, counts


# ----------------------------------------------------------------------------------------
# hand-built rows
# ----------------------------------------------------------------------------------------
def row(*slots):
    """(cand row, col row) of slots (view id, (qR, qG, qB) or None for "no colour"); the keys increase with the slot."""
    c, w = np.full(K, EMPTY, np.int64), np.zeros(K, np.int32)
    for i, (vid, q) in enumerate(slots):
        c[i] = T.make_key(1.0 + 0.125 * i, vid)
        w[i] = 0 if q is None else color_word(q)
    return c, w


def vote(slots, threshold=0.06):
    c, w = row(*slots)
    out, rej, counts = reject_numpy(c[None], w[None], threshold)
    return c, out[0], int(rej[0]), counts.tolist()


GREY, FAR = (400, 400, 400), (1000, 400, 400)


def hand_built_rows():
    """The rows below as one (cand, col) pair, for the GPU test to append to its crafted input."""
    rows = [row((1, (0, 0, 0)), (2, (1020, 1020, 1020))), row(*[(i, GREY) for i in range(5)] + [(9, FAR)]),
            row((9, FAR), *[(i, GREY) for i in range(5)]), row((1, GREY), (2, (400, 461, 400)), (3, (400, 400, 338)), (4, GREY)),
            row((1, (100, 0, 0)), (2, (200, 0, 0)), (3, (300, 0, 0)), (4, (400, 0, 0))),
            row((1, (0, 500, 1000)), (2, (500, 1000, 0)), (3, (1000, 0, 500))), row((1, GREY), (2, None), (3, FAR), (4, None)),
            row((1, GREY), (2, None), (3, GREY), (4, FAR), (5, GREY)), row(), row(*[(i, GREY) for i in range(15)] + [(99, FAR)])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def test_two_views_are_kept_however_far_apart():
    c, out, rej, counts = vote([(1, (0, 0, 0)), (2, (1020, 1020, 1020))])
    assert np.array_equal(out, c) and rej == 0 and counts == [0, 0, 0, 0]


@pytest.mark.parametrize("at", range(6))
def test_one_far_view_of_six_is_removed_wherever_it_sits_and_the_keys_close_up(at):
    slots = [(i, GREY) for i in range(5)]
    slots.insert(at, (9, FAR))
    c, out, rej, counts = vote(slots)
    assert rej == 1 << at and counts == [1, int(at == 0), 1, 0]
    assert np.array_equal(out[:5], np.delete(c[:6], at)) and (out[5:] == EMPTY).all()
    assert (np.diff(out[:5]) > 0).all()


def test_a_deviation_of_t_is_kept_and_of_t_plus_one_removed():
    T_ = int(np.floor(0.06 * QMAX))
    assert T_ == 61 and int(np.floor(1.0 * QMAX)) == 1020 and int(np.floor(0.001 * QMAX)) == 1
    c, out, rej, counts = vote([(1, GREY), (2, (400, 400 + T_, 400)), (3, (400, 400, 400 - T_ - 1)), (4, GREY)])
    assert rej == 0b0100 and counts == [1, 0, 1, 0]
    assert np.array_equal(out[:3], c[[0, 1, 3]])


def test_an_even_number_of_views_takes_the_lower_median():
    # medians of (100, 200, 300, 400) red: lower 200, upper 300; T = 102 separates them: |400 - 200| > 102 >= |400 - 300|
    c, out, rej, counts = vote([(1, (100, 0, 0)), (2, (200, 0, 0)), (3, (300, 0, 0)), (4, (400, 0, 0))], threshold=0.1)
    assert rej == 0b1000 and counts == [1, 0, 1, 0]


def test_a_face_whose_views_are_all_outliers_keeps_them_all():
    slots = [(1, (0, 500, 1000)), (2, (500, 1000, 0)), (3, (1000, 0, 500))]   # the medians (500, 500, 500) belong to three views
    c, w = row(*slots)
    _, n, dev = deviations(c[None], w[None])
    assert n[0] == 3 and (dev[0, :3] == 500).all()
    c, out, rej, counts = vote(slots)
    assert np.array_equal(out, c) and rej == 0 and counts == [1, 0, 0, 1]


def test_a_slot_without_a_colour_is_neither_counted_nor_removed():
    c, out, rej, counts = vote([(1, GREY), (2, None), (3, FAR), (4, None)])   # n = 2
    assert np.array_equal(out, c) and rej == 0 and counts == [0, 0, 0, 0]
    c, out, rej, counts = vote([(1, GREY), (2, None), (3, GREY), (4, FAR), (5, GREY)])   # n = 4: slot 3 goes, slot 1 stays
    assert rej == 0b01000 and np.array_equal(out[:4], c[[0, 1, 2, 4]]) and counts == [1, 0, 1, 0]


def test_an_empty_list_and_a_full_one():
    c, out, rej, counts = vote([])
    assert (out == EMPTY).all() and rej == 0 and counts == [0, 0, 0, 0]
    c, out, rej, counts = vote([(i, GREY) for i in range(15)] + [(99, FAR)])
    assert rej == 1 << 15 and np.array_equal(out[:15], c[:15]) and out[15] == EMPTY


def test_rejecting_slot_0_makes_the_old_second_key_the_choice():
    c, out, rej, counts = vote([(9, FAR)] + [(i, GREY) for i in range(5)])
    assert rej == 1 and out[0] == c[1] and counts == [1, 1, 1, 0]


def test_the_hand_built_rows_cover_every_outcome():
    cand, col = hand_built_rows()
    out, rej, counts = reject_numpy(cand, col, 0.06)
    assert counts.tolist() == [7, 2, 8, 1] and (rej != 0).sum() == 6


# ----------------------------------------------------------------------------------------
# colours
# ----------------------------------------------------------------------------------------
def test_the_colour_of_a_face_is_four_times_the_mean_of_its_four_taps():
    v = T.cam_view(7)   # u = 31.5 + 4 x, v = 23.5 + 4 y
    cand = np.full((1, K), EMPTY, np.int64)
    cand[0, 2] = T.make_key(0.125, 7)
    col = colors_numpy(T.TRI, [[0, 1, 2]], cand, [v])
    assert (col[0, [0, 1] + list(range(3, K))] == 0).all() and col[0, 2] >> 30 == 1
    pu, pv = np.array([31.5, 31.5, 35.5]), np.array([23.5, 27.5, 23.5])
    pts = [(pu.sum() / 3, pv.sum() / 3)] + [((3 * pu[i] + pu.sum()) / 6, (3 * pv[i] + pv.sum()) / 6) for i in range(3)]
    mean = np.mean([tap_numpy(v["image"], np.array([x]), np.array([y]))[0] for x, y in pts], 0)
    assert np.abs(channels(col[0, 2]) - 4 * mean).max() <= 0.5 + 1e-9
    # a view that is not offered, a key of another id and a corner behind the camera leave the slot as it was
    assert (colors_numpy(T.TRI, [[0, 1, 2]], cand, [T.cam_view(8)]) == 0).all()
    behind = T.cam_view(7, C=(0.0, 0.0, 20.0))
    assert (colors_numpy(T.TRI, [[0, 1, 2]], cand, [behind]) == 0).all()
    keep = np.full((1, K), 5, np.int32)
    assert np.array_equal(colors_numpy(T.TRI, [[0, 1, 2]], cand, [behind], keep), keep)
    # a constant image gives four times its colour, exactly
    flat = dict(v, image=np.full_like(v["image"], 0) + np.uint8([10, 200, 255]))
    assert channels(colors_numpy(T.TRI, [[0, 1, 2]], cand, [flat])[0, 2]).tolist() == [40, 800, 1020]


# ----------------------------------------------------------------------------------------
# the behaviour scene
# ----------------------------------------------------------------------------------------
def ramp_image(view, z=10.0):
    """The image of the plane Z = z under the linear world ramp (R, G, B) = (20 + 8 X + 3 Y, 200 - 6 X - 2 Y, 60 + 5 Y + 2 X)."""
    K_, E = view["K"].astype(np.float64), view["E"].astype(np.float64)
    C = -E[:3, 3]
    h, w = view["depth"].shape
    ys, xs = np.mgrid[0:h, 0:w]
    X = C[0] + (xs - K_[0, 2]) / K_[0, 0] * (z - C[2])
    Y = C[1] + (ys - K_[1, 2]) / K_[1, 1] * (z - C[2])
    rgb = np.stack([20 + 8 * X + 3 * Y, 200 - 6 * X - 2 * Y, 60 + 5 * Y + 2 * X], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def behaviour_scene():
    """The 20 x 15 grid at z = 10 (600 faces, x and y jittered by +-0.04) and nine views over it that all show one linear colour
    ramp of the world: honest images agree on every face to within the rounding of a pixel."""
    rng = np.random.default_rng(5)
    nx, ny = 20, 15
    ys, xs = np.mgrid[0:ny + 1, 0:nx + 1]
    V = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 10.0)], 1)
    V[:, :2] += rng.uniform(-0.04, 0.04, (xs.size, 2))
    F = []
    for i in range(ny):
        for j in range(nx):
            a, b, c, d = i * (nx + 1) + j, i * (nx + 1) + j + 1, (i + 1) * (nx + 1) + j, (i + 1) * (nx + 1) + j + 1
            F += [[a, c, b], [b, c, d]]   # normals toward -Z, the cameras
    vs = []
    for k in range(9):
        C = (rng.uniform(4, 16), rng.uniform(3, 12), rng.uniform(0, 0.5))
        v = T.cam_view(k, C=C, f=float(rng.uniform(22, 34)))
        v["depth"][:] = np.float32(10.0 - float(np.float32(C[2])))
        v["image"] = ramp_image(v)
        vs.append(v)
    return V.astype(np.float32), np.array(F, np.int32), vs


def paint(view):
    """A copy of the view with the central half of its image (255, 0, 255)."""
    img = view["image"].copy()
    h, w = img.shape[:2]
    img[h // 4:h - h // 4, w // 4:w - w // 4] = (255, 0, 255)
    return dict(view, image=img)


def winning_view(cand):
    """The id that wins most faces in column 0."""
    ids, n = np.unique(cand[:, 0][cand[:, 0] != EMPTY] & 0xffffffff, return_counts=True)
    return int(ids[np.argmax(n)])


def test_honest_images_reject_nothing_and_a_painted_view_loses_the_faces_it_spoils():
    V, F, vs = behaviour_scene()
    cand = S.candidates_numpy(V, F, vs)
    per_face = (cand != EMPTY).sum(1)
    assert per_face.min() >= 3 and per_face.max() <= 9
    col = colors_numpy(V, F, cand, vs)
    assert np.array_equal(col != 0, cand != EMPTY)
    _, n, dev = deviations(cand, col)
    print("honest: %d .. %d candidates per face, largest deviation %d quarter levels" % (per_face.min(), per_face.max(), dev.max()))
    # a bilinear tap of a linear ramp is exact up to the pixels' rounding (half a grey level), so a colour is within 2 + 0.5 quarter
    # levels of the ramp's and two views within 5 of each other
    assert dev.max() <= 5 < 61
    out, rej, counts = reject_numpy(cand, col, 0.06)
    assert np.array_equal(out, cand) and not rej.any() and counts.tolist() == [600, 0, 0, 0]
    win = winning_view(cand)
    painted = [paint(v) if v["id"] == win else v for v in vs]
    col2 = colors_numpy(V, F, cand, painted)
    out2, rej2, counts2 = reject_numpy(cand, col2, 0.06)
    bits = (rej2[:, None] >> np.arange(K)) & 1
    touched = (col2 != col).any(1)
    print("painted view %d: %d faces touched, %d lose it, %d change their first view" % (win, touched.sum(), (rej2 != 0).sum(), counts2[1]))
    assert not (bits.astype(bool) & (col2 == col)).any()   # no slot whose colour did not change is removed
    first = (bits[:, 0] == 1)
    assert np.array_equal(out2[first, 0], cand[first, 1]) and first.sum() == counts2[1]
    assert (rej2 != 0).sum() > 100 and (rej2 != 0).sum() <= touched.sum()


# ----------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------
NAMES = ["d3d_texture_face_colors", "d3d_texture_outliers"]


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in _lib.SIGNATURES, n
    assert "texture_outliers.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    src = open(os.path.join(_lib.CSRC, "texture_outliers.hip")).read()
    assert "texture_shared.h" in src and "tx_find(" in src and "tx_corner_uv(" in src


def test_the_library_refuses_bad_arguments():
    import ctypes

    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before a launch
    colors = lambda **kw: lib.d3d_texture_face_colors(kw.get("v", p), kw.get("n", 4), kw.get("f", p), kw.get("m", 4), kw.get("cand", p),
                                                      kw.get("views", p), kw.get("nv", 3), kw.get("col", p), None)
    for bad in ({"v": None}, {"f": None}, {"cand": None}, {"col": None}, {"views": None}, {"n": -1}, {"m": -1}, {"nv": -1}, {"m": 1 << 30},
                {"nv": 1 << 20}):
        assert colors(**bad) == -1, bad
    assert colors(m=1 << 30) == -1 and b"n_faces" in lib.d3d_last_error()
    vote = lambda **kw: lib.d3d_texture_outliers(kw.get("cand", p), kw.get("col", p), kw.get("m", 4), kw.get("T", 61), kw.get("out", p),
                                                 kw.get("rej", p), kw.get("counts", p), None)
    for bad in ({"cand": None}, {"col": None}, {"out": None}, {"rej": None}, {"counts": None}, {"m": -1}, {"m": 1 << 30}, {"T": -1},
                {"T": 1021}):
        assert vote(**bad) == -1, bad
    assert vote(T=1021) == -1 and b"T=1021" in lib.d3d_last_error()


def test_settings_and_argument_errors():
    from deep3d_aerial_amd import texture

    assert texture.check_outlier_settings({"threshold": 0.06}) == 0.06
    assert texture.check_outlier_settings({"threshold": 1}) == 1.0
    for bad in ({}, {"threshold": 0}, {"threshold": 1.5}, {"threshold": -0.1}, {"threshold": float("nan")}, {"threshold": float("inf")},
                {"threshold": 0.06, "views": 3}, {"treshold": 0.06}):
        with pytest.raises(ValueError):
            texture.check_outlier_settings(bad)
    base = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in ("0", "1.5", "nan", "-0.06"):
        with pytest.raises(SystemExit):
            texture.main(base + ["--outlier_threshold", bad])
    assert texture.outlier_summary([5, 1, 2, 0], 0.06, 9) == {"threshold": 0.06, "T": 61, "faces": 9, "tested": 5, "changed": 1,
                                                              "removed": 2, "kept_all": 0}
    import torch

    cand, col = torch.zeros((2, K), dtype=torch.int64), torch.zeros((2, K), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.reject_outliers(cand, col, 0.06)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.face_colors(torch.zeros((3, 3)), torch.zeros((2, 3), dtype=torch.int32), cand, [])


def test_the_flag_parses_with_and_without_the_prefix():
    import argparse

    from deep3d_aerial_amd import predict, texture

    ap = argparse.ArgumentParser()
    texture.add_arguments(ap)
    assert texture.settings_from_args(ap.parse_args([]), "o.ply")["outliers"] is None
    s = texture.settings_from_args(ap.parse_args(["--outlier_threshold", "0.06", "--smooth_views", "0.1"]), "o.ply")
    assert s["outliers"] == {"threshold": 0.06} and s["smooth_views"]["weight"] == 0.1
    assert "0.06" in ap.format_help() and "fOutlierThreshold" in ap.format_help()
    base = ["--output_folder", "out", "--synthetic_items", "2", "--random_weights", "--fuse", "--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1",
            "--mesh_voxel=0.5", "--texture", "t.ply"]
    assert predict._texture_settings(predict.parse_args(base))["outliers"] is None
    a = predict.parse_args(base + ["--texture_outlier_threshold", "0.06"])
    assert predict._texture_settings(a)["outliers"] == {"threshold": 0.06}
    for bad in ("0", "1.5", "nan"):
        with pytest.raises(SystemExit):
            predict.parse_args(base + ["--texture_outlier_threshold", bad])
