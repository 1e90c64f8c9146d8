"""The ring kernel's TALL patches (csrc/planesweep_tiled.hip): a last patch column with at most 16 real pixels per row is swept in
16 x 8 patches instead of half-empty 32 x 4 ones.  Per-pixel arithmetic does not depend on the patch a pixel belongs to, so the
forced ring kernel ("tiled") must repeat the window kernel bit for bit (which tiles the map its own way) and match the CPU oracle
within the bounds of test_parity_gpu.test_aggregation_vs_oracle, in every mode and output format the kernel template serves.
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
    # V, C, h, w, D, depth kind, yaw
    (5, 32, 12, 48, 8, "plane", 1.0),     # one wide column + one tall column; three row tiles: a full pair and a half-filled tall patch
    (3, 16, 8, 16, 5, "pixel", 3.0),      # the map is a single tall patch
    (5, 32, 9, 40, 6, "plane", 1.0),      # 8 valid columns of 16, ragged rows
    (5, 32, 16, 33, 4, "plane", 1.0),     # one valid column in the tall patch
    (4, 16, 33, 70, 3, "pixel", 25.0),    # w % 32 = 6 under a big yaw: the tall patch's hull
    (3, 16, 8, 16, 130, "plane", 1.0),    # tall patches across a 128-plane segment boundary
    (2, 32, 37, 53, 5, "plane", 1.0),     # w % 32 = 21: the column stays wide (control)
]
_case_id = lambda c: "V%d_C%d_%dx%d_D%d_%s" % c[:6]
BASE = CASES[0]


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Host inputs of a case (read-only: shared by every test that uses the case)."""
    V, C, h, w, D, kind, yaw = case
    proj, dv = S.make_scene(V, h, w, D, seed=V * 100 + C, yaw_deg=yaw)
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


def _in_domain(path, V, C):
    """launch_window takes C % 8 == 0 and at most 4 source views, launch_tiled C % 8 == 0 and at most 6 (fp32 sweeps)."""
    return C % 8 == 0 and V - 1 <= (4 if path == "window" else 6)


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
def test_tall_patches_repeat_the_window_kernel_and_match_the_oracle(ops, oracle, case):
    V, C, h, w, D, kind, yaw = case
    proj, feats, depth, vw = _scene(case)
    fd = [dev(f) for f in feats]
    p34 = ops.compose_projections(dev(proj))
    p34_host = host(p34).reshape(-1, 3, 4)
    dd, vwd = dev(depth), dev(vw)
    sweep = lambda: (host(ops.variance_volume(fd, p34, dd)), host(ops.weighted_corr(fd, p34, vwd, dd)))
    var, wc = _forced(ops, "tiled", sweep)
    if _in_domain("window", V, C) and _in_domain("tiled", V, C):
        var_w, wc_w = _forced(ops, "window", sweep)
        print("tiled vs window: variance %d, weighted %d voxels differ" % ((var != var_w).sum(), (wc != wc_w).sum()))
        assert np.array_equal(var, var_w)
        assert np.array_equal(wc, wc_w)
    want = oracle.variance_volume(feats[0], feats[1:], p34_host, depth)
    print("variance vs oracle: max abs %.3g, rel-L1 %.3g" % (np.abs(var - want).max(), rel_l1(var, want)))
    assert np.abs(var - want).max() <= 2 * ABS_GATHER
    assert rel_l1(var, want) <= REL_VOLUME
    want = oracle.weighted_corr(feats[0], feats[1:], p34_host, vw, depth)
    print("weighted vs oracle: max abs %.3g, rel-L1 %.3g" % (np.abs(wc - want).max(), rel_l1(wc, want)))
    assert np.abs(wc - want).max() <= 2 * ABS_GATHER
    assert rel_l1(wc, want) <= REL_VOLUME


def test_tall_patches_warp_and_pair_pass(ops, oracle):
    """d3d_homo_warp and d3d_pair_corr_mean (the template's warp and pair modes) on a map with a tall column."""
    proj, feats, depth, _ = _scene(BASE)
    fd = [dev(f) for f in feats]
    p34 = ops.compose_projections(dev(proj))
    p34_host = host(p34).reshape(-1, 3, 4)
    dd = dev(depth)
    wp, pm = _forced(ops, "tiled", lambda: (host(ops.homo_warp(fd[1], p34[0], dd)), host(ops.pair_corr_mean(fd[0], fd[1], p34[0], dd))))
    want = oracle.homo_warp(feats[1], p34_host[0], depth)
    print("warp vs oracle: max abs %.3g" % np.abs(wp - want).max())
    assert np.abs(wp - want).max() <= ABS_GATHER
    want = oracle.pair_corr_mean(feats[0], feats[1], p34_host[0], depth)
    print("pair mean vs oracle: max abs %.3g" % np.abs(pm - want).max())
    assert np.abs(pm - want).max() <= ABS_GATHER


def test_tall_patches_fp16_storage(ops, oracle):
    """fp16 features and cost volume (7 views: the view-major plane loop) on a map with a tall column; the call and the bounds of
    test_parity_gpu.test_variance_volume_fp16_storage_7_views."""
    V, C, h, w, D = 7, 32, 12, 48, 12
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


def test_tall_patches_channel_last_and_plane_major_outputs(ops):
    """The 16-bit channel-last volume in planes of 8-channel groups (CL8) and the plane-major fp32 volume hold the planar
    volume's values: the tall patches' stores go through the same per-lane offsets in every output format."""
    V, C, h, w, D, _, _ = BASE
    proj, feats, depth, _ = _scene(BASE)
    fd = [dev(f) for f in feats]
    p34 = ops.compose_projections(dev(proj))
    dd = dev(depth)
    var, var_pm, cl8 = _forced(ops, "tiled", lambda: (ops.variance_volume(fd, p34, dd), ops.variance_volume(fd, p34, dd, plane_major=True),
                                                      ops.variance_volume_cl(fd, p34, dd, layout="cl8")))
    assert tuple(var_pm.shape) == (D, C, h, w)
    assert np.array_equal(host(var_pm).transpose(1, 0, 2, 3), host(var))
    assert tuple(cl8.shape) == (D, C // 8, h, w, 8)
    assert torch.equal(ops.cl8_to_cl(cl8), var.to(ops.h16_dtype()).permute(1, 2, 3, 0).contiguous())
