"""The true orthophoto on the CPU: a numpy restatement of the semantics in deep3d_aerial_amd/ortho.py (`ortho_numpy`, a brute
force over all views; tests/test_ortho_gpu.py compares the kernels with it bit for bit), checked on hand-built scenes; the
RGBA GeoTIFF writer, the DSM reader, read_red_cam and the argument errors."""
import math
import os

import numpy as np
import pytest
import torch

EMPTY = np.int64((1 << 63) - 1)


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def make_key(s, vid):
    """(bits(fp32(s)) << 32) | id."""
    return (np.asarray(np.float32(s)).view(np.uint32).astype(np.int64) << 32) | np.int64(vid)


def ortho_numpy(height, grid, views, depth_tolerance=0.01):
    """views: [{"id", "K" [3,3], "E" [4,4], "depth" [H,W] fp32, "image" [H,W,3] uint8}].  Returns (key [H,W] int64,
    view [H,W] int32 (-1 empty), rgba [H,W,4] uint8), following the module's semantics literally."""
    H, W = grid.shape
    h = np.asarray(height, np.float32)
    live = np.isfinite(h)
    X0 = np.broadcast_to(grid.x_min + (np.arange(W, dtype=np.float64) + 0.5) * grid.unit[0], (H, W))
    X1 = np.broadcast_to((grid.y_max - (np.arange(H, dtype=np.float64) + 0.5) * grid.unit[1])[:, None], (H, W))
    X2 = np.where(live, h, 0).astype(np.float64)
    key = np.full((H, W), EMPTY, np.int64)
    U = np.zeros((H, W))
    V = np.zeros((H, W))
    for vw in views:
        K = np.asarray(vw["K"], np.float32).astype(np.float64)
        E = np.asarray(vw["E"], np.float32).astype(np.float64)
        R, t = E[:3, :3], E[:3, 3]
        C = [-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)]
        d = np.asarray(vw["depth"], np.float32)
        Hv, Wv = d.shape
        with np.errstate(all="ignore"):
            p0 = R[0, 0] * X0 + R[0, 1] * X1 + R[0, 2] * X2 + t[0]
            p1 = R[1, 0] * X0 + R[1, 1] * X1 + R[1, 2] * X2 + t[1]
            p2 = R[2, 0] * X0 + R[2, 1] * X1 + R[2, 2] * X2 + t[2]
            q0 = K[0, 0] * p0 + K[0, 1] * p1 + K[0, 2] * p2
            q1 = K[1, 0] * p0 + K[1, 1] * p1 + K[1, 2] * p2
            q2 = K[2, 0] * p0 + K[2, 1] * p1 + K[2, 2] * p2
            u = q0 / q2
            v = q1 / q2
            ok = live & (p2 > 0) & (q2 > 0) & (u >= 0) & (u <= Wv - 1) & (v >= 0) & (v <= Hv - 1)
            px = np.where(ok, np.floor(u + 0.5), 0).astype(np.int64)
            py = np.where(ok, np.floor(v + 0.5), 0).astype(np.int64)
            D = d[py, px]
            ok &= np.isfinite(D) & (D > 0) & (p2 <= D.astype(np.float64) * (1.0 + depth_tolerance))
            dx, dy, dz = X0 - C[0], X1 - C[1], X2 - C[2]
            s = (dx * dx + dy * dy) / (dz * dz)
            ok &= np.isfinite(s)
            k = make_key(np.where(ok, s, 0.0), vw["id"])
        better = ok & (k < key)
        key[better] = k[better]
        U[better] = u[better]
        V[better] = v[better]
    view = np.where(key == EMPTY, -1, key & 0xffffffff).astype(np.int32)
    rgba = np.zeros((H, W, 4), np.uint8)
    by_id = {int(vw["id"]): vw for vw in views}
    for vid in np.unique(view[view >= 0]):
        m = view == vid
        img = np.asarray(by_id[int(vid)]["image"], np.uint8)
        Hv, Wv = img.shape[:2]
        u, v = U[m], V[m]
        fu, fv = np.floor(u), np.floor(v)
        fx, fy = u - fu, v - fv
        x0, y0 = np.minimum(fu.astype(np.int64), Wv - 1), np.minimum(fv.astype(np.int64), Hv - 1)
        x1, y1 = np.minimum(x0 + 1, Wv - 1), np.minimum(y0 + 1, Hv - 1)
        w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
        out = np.empty((len(u), 4), np.uint8)
        for ch in range(3):
            c = img[:, :, ch].astype(np.float64)
            val = w00 * c[y0, x0] + w10 * c[y0, x1] + w01 * c[y1, x0] + w11 * c[y1, x1]
            out[:, ch] = np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
        out[:, 3] = 255
        rgba[m] = out
    return key, view, rgba


# ----------------------------------------------------------------------------------------
# scenes: flat ground plus boxes, cameras looking along +Z (Z points away from them), ray-cast analytically
# ----------------------------------------------------------------------------------------
GROUND = 100.0


def texture(x, y):
    """A smooth colour field over the world plane (small gradients: the bilinear error stays below one level)."""
    r = 128 + 100 * np.sin(x / 9.0)
    g = 128 + 100 * np.cos(y / 7.0)
    b = 128 + 60 * np.sin((x + y) / 11.0)
    return np.stack([r, g, b], -1)


def camera(C, f, w, h, tilt=(0.0, 0.0)):
    """K, E = Tcw (float32) of a camera at C whose optical axis is +Z tilted by `tilt` radians about X then Y."""
    ax, ay = tilt
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rcw = (Ry @ Rx).T
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = Rcw
    E[:3, 3] = -Rcw @ np.asarray(C, np.float64)
    return K.astype(np.float32), E.astype(np.float32)


def render(K, E, w, h, boxes, roof_tex=lambda x, y: texture(x + 50.0, y - 30.0)):
    """(depth [h,w] fp32, image [h,w,3] uint8) of ground z = GROUND and boxes [(x0, x1, y0, y1, z_top)] (each from z_top down
    to the ground) seen by the camera: the nearest hit along every pixel's ray."""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    C = -R.T @ t
    ys, xs = np.mgrid[0:h, 0:w]
    rc = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])   # camera rays with z = 1: the parameter is the depth
    d = (R.T @ rc).T
    with np.errstate(all="ignore"):
        lam = (GROUND - C[2]) / d[:, 2]
    lam = np.where(lam > 0, lam, np.inf)
    which = np.full(h * w, -1)
    for b, (bx0, bx1, by0, by1, top) in enumerate(boxes):
        lo = np.array([bx0, by0, top])
        hi = np.array([bx1, by1, GROUND])
        with np.errstate(all="ignore"):
            t0 = (lo - C) / d
            t1 = (hi - C) / d
        tn = np.nanmax(np.minimum(t0, t1), 1)
        tf = np.nanmin(np.maximum(t0, t1), 1)
        hit = (tn <= tf) & (tn > 0) & (tn < lam)
        lam = np.where(hit, tn, lam)
        which = np.where(hit, b, which)
    P = C + lam[:, None] * d
    with np.errstate(all="ignore"):
        col = np.where((which >= 0)[:, None], roof_tex(P[:, 0], P[:, 1]), texture(P[:, 0], P[:, 1]))
    depth = np.where(np.isfinite(lam), lam, 0.0).reshape(h, w).astype(np.float32)
    img = np.clip(np.floor(np.nan_to_num(col) + 0.5), 0, 255).astype(np.uint8).reshape(h, w, 3)
    return depth, img


def dsm_of(grid, boxes):
    """The DSM of the scene at the cell centres: the top of the box a centre lies in, else the ground."""
    H, W = grid.shape
    x = grid.x_min + (np.arange(W) + 0.5) * grid.unit[0]
    y = grid.y_max - (np.arange(H) + 0.5) * grid.unit[1]
    X, Y = np.meshgrid(x, y)
    h = np.full((H, W), GROUND, np.float32)
    for bx0, bx1, by0, by1, top in boxes:
        h[(X >= bx0) & (X <= bx1) & (Y >= by0) & (Y <= by1)] = top
    return h


def view(vid, C, boxes, w=160, h=120, f=100.0, tilt=(0.0, 0.0)):
    K, E = camera(C, f, w, h, tilt)
    depth, img = render(K, E, w, h, boxes)
    return {"id": vid, "K": K, "E": E, "depth": depth, "image": img}


BOX = (-5.0, 5.0, -6.0, 6.0, 80.0)


def _grid():
    from deep3d_aerial_amd import dsm

    return dsm.DsmGrid([-40.0, 40.0, -20.0, 20.0], [0.5, 0.5])


def _centres(grid):
    H, W = grid.shape
    x = grid.x_min + (np.arange(W) + 0.5) * grid.unit[0]
    y = grid.y_max - (np.arange(H) + 0.5) * grid.unit[1]
    return np.meshgrid(x, y)


def test_hidden_ground_takes_the_other_camera_and_shared_ground_the_more_nadir():
    grid = _grid()
    views = [view(1, (-60.0, 0.0, 0.0), [BOX]), view(2, (60.0, 0.0, 0.0), [BOX])]
    key, vid, rgba = ortho_numpy(dsm_of(grid, [BOX]), grid, views)
    X, Y = _centres(grid)
    ground = (np.abs(Y) < 5.0)
    # the ground just east of the box is hidden from camera 1 (west) by the roof: camera 2
    hidden_from_1 = ground & (X > 6.0) & (X < 11.0)
    assert hidden_from_1.sum() > 20 and (vid[hidden_from_1] == 2).all()
    hidden_from_2 = ground & (X < -6.0) & (X > -11.0)
    assert hidden_from_2.sum() > 20 and (vid[hidden_from_2] == 1).all()
    # both see it: the more nadir camera (the nearer one in x)
    assert (vid[ground & (X < -15.0)] == 1).all() and (vid[ground & (X > 15.0)] == 2).all()
    assert (vid >= 0).all() and (rgba[..., 3] == 255).all()
    # the colour is the texture of the ground within the bilinear error
    tex = texture(X, Y)
    far = ground & (np.abs(X) > 12.0)
    assert np.abs(rgba[far][:, :3].astype(float) - tex[far]).max() <= 3.0


def test_an_exact_tie_goes_to_the_lower_id():
    grid = _grid()
    a = view(7, (0.0, 0.0, 0.0), [BOX])
    b = dict(a, id=3)
    key, vid, _ = ortho_numpy(dsm_of(grid, [BOX]), grid, [a, b])
    seen = vid >= 0
    assert seen.mean() > 0.9 and (vid[seen] == 3).all()
    key2, vid2, _ = ortho_numpy(dsm_of(grid, [BOX]), grid, [b, a])
    assert np.array_equal(key, key2)


def test_cells_behind_a_camera_or_outside_its_image_get_no_view():
    grid = _grid()
    h = dsm_of(grid, [])
    behind = view(4, (0.0, 0.0, 150.0), [])             # above the ground on the far side: every cell is behind it
    assert ortho_numpy(h, grid, [behind])[1].max() == -1
    narrow = view(5, (0.0, 0.0, 0.0), [], w=40, h=30)    # sees |x| <= 20, |y| <= 15 of the ground
    key, vid, rgba = ortho_numpy(h, grid, [narrow])
    X, Y = _centres(grid)
    inside = (np.abs(X) < 19.0) & (np.abs(Y) < 14.0)
    outside = (np.abs(X) > 21.0) | (np.abs(Y) > 16.0)
    assert (vid[inside] == 5).all() and (vid[outside] == -1).all()
    assert (key[outside] == EMPTY).all() and (rgba[outside] == 0).all()
    # empty DSM cells stay empty
    h[3:9, 10:30] = np.nan
    key, vid, rgba = ortho_numpy(h, grid, [narrow])
    assert (key[3:9, 10:30] == EMPTY).all() and (rgba[3:9, 10:30] == 0).all()


def test_key_is_monotone_in_the_score_and_int64_max_when_empty():
    rng = np.random.default_rng(3)
    s = np.concatenate([[0.0, 1e-30, 1.0, 1.0, 3e38], rng.uniform(0, 10, 200) ** 3])
    ids = rng.integers(0, 1 << 31 - 1, len(s))
    keys = np.array([make_key(a, i) for a, i in zip(s, ids)])
    order_key = np.argsort(keys, kind="stable")
    order_sem = sorted(range(len(s)), key=lambda k: (np.float32(s[k]), ids[k]))
    assert [int(keys[k]) for k in order_key] == [int(keys[k]) for k in order_sem]
    assert (keys >= 0).all() and (keys < EMPTY).all()
    grid = _grid()
    h = np.full(grid.shape, np.nan, np.float32)
    key, vid, _ = ortho_numpy(h, grid, [view(1, (0.0, 0.0, 0.0), [])])
    assert (key == EMPTY).all() and (vid == -1).all()


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def test_write_ortho_is_an_rgba_tiff_with_the_dsm_world_file(tmp_path):
    from PIL import Image
    from deep3d_aerial_amd import dsm, ortho

    grid = dsm.DsmGrid([100.0, 137.0, -20.0, 3.0], [0.5, 0.25])
    rgba = np.random.default_rng(1).integers(0, 256, grid.shape + (4,), dtype=np.uint8)
    tif, tfw = ortho.write_ortho(str(tmp_path / "o.tif"), rgba, grid)
    im = Image.open(tif)
    assert im.mode == "RGBA" and im.size == (grid.width, grid.height)
    assert np.array_equal(np.array(im), rgba)
    dsm.write_dsm(str(tmp_path / "d.tif"), np.zeros(grid.shape, np.float32), grid)
    assert open(tfw).read() == (tmp_path / "d.tfw").read_text() == grid.tfw_text()
    # the GeoTIFF tags are the DSM file's, GDAL_NODATA is not there
    t = dsm._ifd(open(tif, "rb").read(), tif)
    d = dsm._ifd((tmp_path / "d.tif").read_bytes(), "d")
    for tag in (33550, 33922, 34735):
        assert t[tag] == d[tag]
    assert 42113 not in t and t[262] == [2] and t[338] == [2] and t[277] == [4]
    with pytest.raises(ValueError, match="end in .tif"):
        ortho.write_ortho(str(tmp_path / "o.png"), rgba, grid)
    with pytest.raises(ValueError, match="4 GiB"):
        ortho.write_ortho(str(tmp_path / "big.tif"), rgba, dsm.DsmGrid([0, 1, 0, 1], [1, 1], size=(40000, 30000)))


def test_read_dsm_returns_what_write_dsm_wrote(tmp_path):
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid([-20.0, 40.0, 3.0, 28.0], [0.5, 0.25])
    h = np.random.default_rng(2).uniform(-50, 50, grid.shape).astype(np.float32)
    h[5:9, 7:20] = np.nan
    h[0, 0] = -0.0
    dsm.write_dsm(str(tmp_path / "d.tif"), h, grid)
    h2, g2 = dsm.read_dsm(str(tmp_path / "d.tif"))
    assert g2 == grid and g2.tfw_text() == grid.tfw_text()
    assert np.array_equal(np.isnan(h2), np.isnan(h))
    assert np.array_equal(h2[~np.isnan(h)].view(np.uint32), h[~np.isnan(h)].view(np.uint32))
    # other layouts are refused
    from PIL import Image

    Image.fromarray(np.zeros((4, 5), np.uint8)).save(str(tmp_path / "u8.tif"))
    with pytest.raises(ValueError, match="not a DSM file"):
        dsm.read_dsm(str(tmp_path / "u8.tif"))
    (tmp_path / "junk.tif").write_bytes(b"MM\0*" + b"\0" * 20)
    with pytest.raises(ValueError, match="little-endian classic TIFF"):
        dsm.read_dsm(str(tmp_path / "junk.tif"))


def test_read_red_cam_inverts_write_red_cam(tmp_path):
    from deep3d_aerial_amd import predict

    rng = np.random.default_rng(4)
    cam = rng.standard_normal((2, 4, 4)).astype(np.float32) * np.float32(123.456)
    loc = ["3584", "4096", "17", "IMG_0017.jpg"]
    predict.write_red_cam(str(tmp_path / "c.txt"), cam, loc, "/data/img dir/IMG_0017.jpg")
    got, loc2, path = predict.read_red_cam(str(tmp_path / "c.txt"))
    assert np.array_equal(got[0], cam[0]) and np.array_equal(got[1, :3, :3], cam[1, :3, :3])
    assert np.array_equal(got[1, 3], cam[1, 3])
    assert loc2 == loc and path == "/data/img dir/IMG_0017.jpg"
    (tmp_path / "bad.txt").write_text("hello\n")
    with pytest.raises(ValueError, match="camera file"):
        predict.read_red_cam(str(tmp_path / "bad.txt"))


# ----------------------------------------------------------------------------------------
# argument errors
# ----------------------------------------------------------------------------------------
def test_argument_errors(capsys):
    from deep3d_aerial_amd import dsm, mvs_dl, ortho, pipeline, predict

    base = ["--output_folder", "x", "--synthetic_items", "2"]
    with pytest.raises(SystemExit):
        predict.parse_args(base + ["--ortho", "o.tif"])
    assert "--ortho needs --fuse" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse_args(base + ["--fuse", "--ortho", "o.tif"])
    assert "--ortho needs --dsm" in capsys.readouterr().err
    dsm_args = ["--fuse", "--dsm", "d.tif", "--dsm_border", "0,1,0,1", "--ortho", "o.tif"]
    with pytest.raises(SystemExit):
        predict.parse_args(base + dsm_args + ["--ortho_depth_tolerance=-0.5"])
    assert "depth_tolerance" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict.parse_args(base + dsm_args + ["--ortho_views_per_batch=0"])
    assert "views_per_batch" in capsys.readouterr().err
    a = predict.parse_args(base + dsm_args + ["--ortho_depth_tolerance=0.02", "--ortho_views_per_batch=8"])
    assert predict._ortho_settings(a) == {"path": "o.tif", "depth_tolerance": 0.02, "views_per_batch": 8}
    with pytest.raises(ValueError, match="ortho needs dsm"):
        pipeline.predict_and_fuse(None, [], "x", ortho={"path": "o.tif"})
    with pytest.raises(ValueError, match="depth_tolerance"):
        pipeline.predict_and_fuse(None, [], "x", dsm={"path": "d.tif"}, ortho={"path": "o.tif", "depth_tolerance": math.nan})
    with pytest.raises(ValueError, match="dsm settings"):
        mvs_dl.MVS_Inference(96, 64, pretrain_weight="w.ckpt", ortho={"path": "o.tif"}).argv("in", "out")
    argv = mvs_dl.MVS_Inference(96, 64, pretrain_weight="w.ckpt", dsm={"path": "d.tif", "border": [0, 1, 0, 1]},
                                ortho={"path": "o.tif", "depth_tolerance": 0.01}).argv("in", "out")
    assert "--ortho=o.tif" in argv and not any(x.startswith("--ortho_") for x in argv)
    # image and depth sizes that differ: a camera file's image smaller than its depth map is refused
    with pytest.raises(ValueError, match="smaller than"):
        ortho.center_crop(np.zeros((30, 40, 3), np.uint8), 32, 40)
    crop = ortho.center_crop(np.arange(7 * 9).reshape(7, 9), 4, 6)
    assert crop[0, 0] == 2 * 9 + 2   # start ceil((7 - 4) / 2) = 2, ceil((9 - 6) / 2) = 2, as dataset.crop_window
    # CPU tensors are refused (no fallback)
    grid = dsm.DsmGrid([0.0, 4.0, 0.0, 4.0], [1.0, 1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ortho.select_views(torch.zeros(4, 4), grid, [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ortho.OrthoView(0, np.eye(3), np.eye(4), torch.ones(4, 4), torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="view id"):
        ortho.OrthoView(-1, np.eye(3), np.eye(4), torch.ones(4, 4), torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="depth_tolerance"):
        ortho.check_tolerance(-1.0)
