"""Ties tests/sweep_ref.py (the plane sweeps in float64) down on the CPU: against the reference's own fp32 outputs
(tests/golden/ops_warp.npz, ops_aggregate.npz), against ATen's grid_sample in float64 (the tap and padding rule, independently of
both oracles), against the C oracle on every case tests/test_sweep_views_gpu.py runs, and against the closed forms of the
degenerate views.

Bounds.  The restatement is exact to ~1e-15; what it is compared with is fp32 arithmetic on white-noise features, whose coordinate
rounding (~3e-5 px) gives ~6e-5 max abs and ~3e-6 relative L1 on a variance volume (measured over V = 2 .. 16, C = 5 .. 48).  The
fp32 comparisons are held to a quarter of the kernels' bounds (test_parity_gpu.ABS_GATHER, REL_VOLUME): a failure here means the
restatement is wrong, and the kernels' bounds carry over unchanged to the kernel-against-float64 comparison."""
import numpy as np
import pytest
import torch

import sweep_ref as R
from conftest import load_golden

ABS_VOLUME = 5e-4        # a quarter of 2 * ABS_GATHER
REL_VOLUME = 1.25e-5     # a quarter of REL_VOLUME
ABS_WARP = 2.5e-4        # a quarter of ABS_GATHER (warp, pair mean)


def _held(name, got, want, abs_bound, rel_bound=None):
    err, rel = float(np.abs(got - want).max()), R.rel_l1(got, want)
    print("%s: max abs %.3g, rel-L1 %.3g" % (name, err, rel))
    assert got.shape == want.shape
    assert err <= abs_bound, name
    assert rel_bound is None or rel <= rel_bound, name


def _proj34(oracle, proj):
    return np.stack([oracle.compose_proj(proj[i], proj[0]) for i in range(1, proj.shape[0])])


# ----------------------------------------------------------------------------------------
# the reference's own outputs
# ----------------------------------------------------------------------------------------
def test_warp_golden():
    g = load_golden("ops_warp")
    n = int(g["n_cases"])
    for i in range(n):
        k = "c%d_" % i
        got = R.warp(g[k + "src"], g[k + "proj34"], g[k + "depth"])
        _held("warp golden %d" % i, got, g[k + "out"], ABS_WARP)
    assert n >= 10


def test_aggregation_golden():
    g = load_golden("ops_aggregate")
    n = int(g["n_cases"])
    for i in range(n):
        k = "c%d_" % i
        feats, p34, depth = g[k + "feats"], g[k + "proj34"], g[k + "depth"]
        _held("variance golden %d" % i, R.variance_volume(feats, p34, depth), g[k + "variance"], ABS_VOLUME, REL_VOLUME)
        _held("weighted golden %d" % i, R.weighted_corr(feats, p34, g[k + "weights"], depth), g[k + "weighted"], ABS_VOLUME, REL_VOLUME)
        for j in range(feats.shape[0] - 1):
            _held("pair mean golden %d/%d" % (i, j), R.pair_corr_mean(feats[0], feats[j + 1], p34[j], depth), g[k + "pair_mean"][j], ABS_WARP)
    assert n >= 1


# ----------------------------------------------------------------------------------------
# ATen
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", [(R.FP32_ROWS[0], "pixel"), (R.FP32_ROWS[3], "plane"), (R.FP32_ROWS[4], "affine")],
                         ids=lambda p: p if isinstance(p, str) else "V%d_C%d" % p[:2])
def test_warp_is_grid_sample_in_float64(oracle, row, kind):
    """F.grid_sample(bilinear, zeros, align_corners=True) on the normalised float64 grid of module.py:548-553."""
    sc = R.fp32_scene(row, kind)
    p34 = _proj34(oracle, sc.proj).astype(np.float64)
    # the last view also pushed half out of frame, so that every border and the far-outside rule are sampled
    p34[-1, 0] += 0.6 * sc.w * p34[-1, 2]       # u + 0.6 w
    dv = R.depth_planes(sc.depth, sc.h, sc.w)
    worst = 0.0
    for i in range(sc.V - 1):
        u, v = R.project(p34[i], dv)
        grid = np.stack([u / ((sc.w - 1) / 2.0) - 1.0, v / ((sc.h - 1) / 2.0) - 1.0], -1).reshape(1, sc.D * sc.h, sc.w, 2)
        src = torch.from_numpy(np.asarray(sc.feats[i + 1], np.float64))[None]
        want = torch.nn.functional.grid_sample(src, torch.from_numpy(grid), mode="bilinear", padding_mode="zeros", align_corners=True)
        want = want[0].numpy().reshape(sc.C, sc.D, sc.h, sc.w)
        got = R.sample(sc.feats[i + 1], u, v)
        assert np.array_equal(got, R.warp(sc.feats[i + 1], p34[i], sc.depth))
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        if i == sc.V - 2:
            assert 0.2 < float((want == 0).mean()) < 0.95      # the shifted view is partly, not wholly, out of frame
    print("warp vs grid_sample (float64): %.3g relative" % worst)
    assert worst <= 1e-12


def test_sample_border_taps_and_non_finite_positions():
    src = np.ones((2, 4, 6))
    u = np.array([-0.5, 5.5, 2.0, 2.0, -1.0, 6.0, np.inf, np.nan, 1e300, 2.25])
    v = np.array([1.0, 1.0, -0.25, 3.75, 1.0, 1.0, 1.0, 1.0, 1.0, -np.inf])
    assert np.array_equal(R.sample(src, u, v)[0], [0.5, 0.5, 0.75, 0.25, 0, 0, 0, 0, 0, 0])


# ----------------------------------------------------------------------------------------
# the C oracle, on every case of the GPU tests
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", [pytest.param(r, k, id=R.fp32_id(r, k)) for r in R.FP32_ROWS for k in R.DEPTH_KINDS])
def test_fp32_cases_against_the_oracle(oracle, row, kind):
    sc = R.fp32_scene(row, kind)
    p34, d32 = _proj34(oracle, sc.proj), sc.depth_f32()
    _held("variance", R.variance_volume(sc.feats, p34, sc.depth), oracle.variance_volume(sc.feats[0], sc.feats[1:], p34, d32),
          ABS_VOLUME, REL_VOLUME)
    _held("weighted", R.weighted_corr(sc.feats, p34, sc.weights, sc.depth),
          oracle.weighted_corr(sc.feats[0], sc.feats[1:], p34, sc.weights, d32), ABS_VOLUME, REL_VOLUME)
    j = sc.V - 2
    _held("warp", R.warp(sc.feats[j + 1], p34[j], sc.depth), oracle.homo_warp(sc.feats[j + 1], p34[j], d32), ABS_WARP)
    _held("pair mean", R.pair_corr_mean(sc.feats[0], sc.feats[1], p34[0], sc.depth),
          oracle.pair_corr_mean(sc.feats[0], sc.feats[1], p34[0], d32), ABS_WARP)


@pytest.mark.parametrize("row", R.FP16_ROWS, ids=R.fp16_id)
def test_fp16_cases_against_the_oracle(oracle, row):
    """The fp16-valued features, widened: to float64 for the restatement, to fp32 for the oracle."""
    sc = R.fp16_scene(row)
    assert sc.feats.dtype == np.float16
    p34 = _proj34(oracle, sc.proj)
    f = sc.feats.astype(np.float32)
    want = oracle.variance_volume(f[0], f[1:], p34, sc.depth_f32())
    got = R.variance_volume(sc.feats, p34, sc.depth)
    _held("variance", got, want, ABS_VOLUME, REL_VOLUME)
    print("fp16 roundings that differ, oracle vs float64: %.3g %%" % (100.0 * np.mean(want.astype(np.float16) != got.astype(np.float16))))


def test_affine_planes_are_the_fp32_volume():
    """plane k = fl(lo + fl(k * step)): both roundings, on values where a fused or float64 evaluation differs."""
    sc = R.fp32_scene(R.FP32_ROWS[1], "affine")
    lo, step, D = sc.depth
    vol = R.depth_planes(sc.depth, sc.h, sc.w)
    k = np.arange(D, dtype=np.float32).reshape(-1, 1, 1)
    assert np.array_equal(vol, (lo[None] + k * step[None]).astype(np.float64))      # numpy keeps fp32 between the two operations
    exact = lo.astype(np.float64)[None] + k.astype(np.float64) * step.astype(np.float64)[None]
    assert (vol != exact).mean() > 0.3 and np.abs(vol - exact).max() <= 2.0 ** -23 * np.abs(exact).max()
    assert np.array_equal(sc.depth_f32().astype(np.float64), vol)


# ----------------------------------------------------------------------------------------
# degenerate source views: the closed forms
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,noise", [(8, False), (16, True)], ids=["C8_constant", "C16_noise"])
def test_degenerate_views_closed_forms(oracle, C, noise):
    feats, wts = R.degenerate_feats(C, noise), R.degenerate_weights()
    variance, weighted, pair = R.degenerate_closed_forms(feats, wts)
    p34, depth = R.DEGENERATE_PROJ, R.DEGENERATE_DEPTH
    got = R.variance_volume(feats, p34, depth)
    assert np.isfinite(got).all() and np.abs(got - variance).max() <= 1e-12 * np.abs(variance).max()
    got = R.weighted_corr(feats, p34, wts, depth)
    assert np.isfinite(got).all() and np.abs(got - weighted).max() <= 1e-12 * np.abs(weighted).max()
    for i in range(3):
        got = R.pair_corr_mean(feats[0], feats[i + 1], p34[i], depth)
        assert np.isfinite(got).all() and np.abs(got - pair[i]).max() <= 1e-12 * max(np.abs(pair[i]).max(), 1.0)
        if i != R.DEGENERATE_IDENTITY:
            assert np.count_nonzero(got) == 0 and np.count_nonzero(R.warp(feats[i + 1], p34[i], depth)) == 0
        _held("pair mean %d" % i, pair[i], oracle.pair_corr_mean(feats[0], feats[i + 1], p34[i], depth), ABS_WARP)
    _held("variance", variance, oracle.variance_volume(feats[0], feats[1:], p34, depth), ABS_VOLUME, REL_VOLUME)
    _held("weighted", weighted, oracle.weighted_corr(feats[0], feats[1:], p34, wts, depth), ABS_VOLUME, REL_VOLUME)
