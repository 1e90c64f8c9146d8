"""The ring kernel's staging path (csrc/planesweep_tiled.hip: item, put, write_round, stage).  A staging item -- 64 ring positions
of a step's flattened delta -- that lies inside one rectangle is decoded once per wave (descriptor and ring geometry in scalar
registers, a 32-bit source offset against a wave-uniform base), written without the zero selects when it lies inside the image and
without the duplicate writes when it meets neither ring column 0 nor ring row 0; an item that spans several rectangles takes the
per-lane decode.  Which path staged a position must not show in the rings: the forced ring kernel ("tiled") repeats the window
kernel bit for bit where both serve the case and matches the CPU oracle within the bounds of test_parity_gpu.

The cases, by what they stage:
  * D >= 96: the loaders read the channel-last copy of the maps; below, the planar maps (no workspace copy);
  * first windows (whole rectangles: one-rectangle items) next to thin L-shaped deltas (items across several rectangles);
  * three sources on the four-view template (the zeroed slot of the copy), windows that leave the image on every side (border
    items beside interior ones);
  * rings that wrap, so that the duplicate column and row are written, across a 128-plane segment boundary;
  * fp16 storage (8-word ring positions, view-major kernel);
  * the weighted, warp and pair modes of the template.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l1
from deep3d_aerial_amd import config, synthetic as S

pytestmark = pytest.mark.gpu

ABS_GATHER = 1e-3     # max abs error of a warped N(0,1) white-noise feature (test_parity_gpu.ABS_GATHER)
REL_VOLUME = 5e-5     # relative L1 of a whole cost volume (test_parity_gpu.REL_VOLUME)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deep3d_aerial_amd import _lib, ops as _ops

    _lib.load()  # raises if the HIP library is missing: no silent fallback
    return _ops


@pytest.fixture(autouse=True)
def _dispatcher_chooses_again():
    """No test leaves a kernel family forced behind it."""
    yield
    config.switches["D3D_FORCE_PATH"] = ""


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()   # (a copy: the shared host inputs are read-only)


def host(t):
    return t.detach().cpu().numpy()


CASES = [
    # V, C, h, w, D, depth kind, yaw, sweep_px
    (5, 32, 24, 80, 100, "plane", 1.0, None),    # channel-last copy, two channel groups, several steps
    (4, 16, 20, 72, 100, "plane", 25.0, 48.0),   # three sources on the four-view template; windows leave the image on all sides
    (5, 16, 40, 96, 24, "pixel", 1.0, None),     # planar staging (no workspace copy)
    (3, 16, 8, 16, 130, "plane", 1.0, None),     # wrapping rings, duplicate column and row, a 128-plane segment boundary
]
_case_id = lambda c: "V%d_C%d_%dx%d_D%d_%s" % c[:6]
BASE = CASES[0]


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Host inputs of a case (read-only: shared by every test that uses the case)."""
    V, C, h, w, D, kind, yaw, sweep_px = case
    proj, dv = S.make_scene(V, h, w, D, sweep_px=sweep_px, seed=V * 100 + C, yaw_deg=yaw)
    feats = S.make_features(V, C, h, w, seed=C + D)
    rng = np.random.default_rng(D)
    if kind == "plane":
        depth = S.uniform_depths(dv, D)
    else:
        depth = np.sort(rng.uniform(dv[0], dv[1], (D, h, w)).astype(np.float32), 0)
    vw = rng.uniform(0.02, 1.0, (V - 1, h, w)).astype(np.float32)
    for a in (proj, feats, depth, vw):
        a.setflags(write=False)
    return proj, feats, depth, vw


def _forced(ops, path, fn):
    """fn() with one kernel family forced; asserts that this family is the one that ran."""
    config.switches["D3D_FORCE_PATH"] = path
    try:
        ops.sweep_dispatch_counts(reset=True)
        out = fn()
        counts = ops.sweep_dispatch_counts()
    finally:
        config.switches["D3D_FORCE_PATH"] = ""
    assert counts[path] > 0, counts
    assert all(n == 0 for k, n in counts.items() if k != path and k in ("direct", "tiled", "window")), counts
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_staged_rings_repeat_the_window_kernel_and_match_the_oracle(ops, oracle, case):
    V, C, h, w, D, kind, yaw, _ = case
    proj, feats, depth, vw = _scene(case)
    fd = [dev(f) for f in feats]
    p34 = ops.compose_projections(dev(proj))
    p34_host = host(p34).reshape(-1, 3, 4)
    dd = dev(depth)
    sweep = lambda: host(ops.variance_volume(fd, p34, dd))
    var = _forced(ops, "tiled", sweep)
    var_w = _forced(ops, "window", sweep)   # (every case has C % 8 == 0 and at most 4 sources: both families serve it)
    print("tiled vs window: %d voxels differ" % (var != var_w).sum())
    assert np.array_equal(var, var_w)
    want = oracle.variance_volume(feats[0], feats[1:], p34_host, depth)
    print("variance vs oracle: max abs %.3g, rel-L1 %.3g" % (np.abs(var - want).max(), rel_l1(var, want)))
    assert np.abs(var - want).max() <= 2 * ABS_GATHER
    assert rel_l1(var, want) <= REL_VOLUME


def test_staged_rings_weighted_warp_and_pair_pass(ops, oracle):
    """d3d_weighted_corr, d3d_homo_warp and d3d_pair_corr_mean (the template's other modes) on the first case's scene."""
    proj, feats, depth, vw = _scene(BASE)
    fd = [dev(f) for f in feats]
    p34 = ops.compose_projections(dev(proj))
    p34_host = host(p34).reshape(-1, 3, 4)
    dd, vwd = dev(depth), dev(vw)
    weighted = lambda: host(ops.weighted_corr(fd, p34, vwd, dd))
    wc = _forced(ops, "tiled", weighted)
    wc_w = _forced(ops, "window", weighted)
    print("weighted, tiled vs window: %d voxels differ" % (wc != wc_w).sum())
    assert np.array_equal(wc, wc_w)
    want = oracle.weighted_corr(feats[0], feats[1:], p34_host, vw, depth)
    print("weighted vs oracle: max abs %.3g, rel-L1 %.3g" % (np.abs(wc - want).max(), rel_l1(wc, want)))
    assert np.abs(wc - want).max() <= 2 * ABS_GATHER
    assert rel_l1(wc, want) <= REL_VOLUME
    wp, pm = _forced(ops, "tiled", lambda: (host(ops.homo_warp(fd[1], p34[0], dd)), host(ops.pair_corr_mean(fd[0], fd[1], p34[0], dd))))
    want = oracle.homo_warp(feats[1], p34_host[0], depth)
    print("warp vs oracle: max abs %.3g" % np.abs(wp - want).max())
    assert np.abs(wp - want).max() <= ABS_GATHER
    want = oracle.pair_corr_mean(feats[0], feats[1], p34_host[0], depth)
    print("pair mean vs oracle: max abs %.3g" % np.abs(pm - want).max())
    assert np.abs(pm - want).max() <= ABS_GATHER


def test_staged_rings_fp16_storage(ops, oracle):
    """fp16 features and cost volume (7 views: 8-word ring positions, the view-major plane loop); the call and the bounds of
    test_sweep_ragged_gpu.test_tall_patches_fp16_storage."""
    V, C, h, w, D = 7, 32, 24, 80, 12
    proj, dv = S.make_scene(V, h, w, D, sweep_px=6.0, seed=77, yaw_deg=4.0)
    feats = [f.astype(np.float16) for f in S.make_features(V, C, h, w, seed=7)]
    depth = S.uniform_depths(dv, D)
    p34 = ops.compose_projections(dev(proj))
    got = _forced(ops, "tiled", lambda: ops.variance_volume([torch.from_numpy(f).cuda() for f in feats], p34, dev(depth)))
    assert got.dtype == torch.float16 and tuple(got.shape) == (C, D, h, w)
    f32 = [f.astype(np.float32) for f in feats]
    want = oracle.variance_volume(f32[0], f32[1:], host(p34).reshape(-1, 3, 4), depth)
    g = got.float().cpu().numpy()
    print("fp16 storage vs oracle: max abs %.3g of %.3g" % (np.abs(g - want).max(), np.abs(want).max()))
    # one fp16 rounding of a value that the fp32 kernel reproduces to ~1e-6: half an ulp of fp16 plus slack
    assert np.abs(g - want).max() <= 2.0 ** -10 * np.abs(want).max() + 1e-6
    assert np.abs(g - want.astype(np.float16).astype(np.float32)).mean() <= 1e-4 * np.abs(want).mean()
