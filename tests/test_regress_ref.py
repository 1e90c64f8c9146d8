"""The float64 restatements of tests/regress_ref.py against the reference itself: its own fp32 outputs (tests/golden) and ATen's
bilinear interpolation on the CPU.  No GPU and no code under test: this is what entitles tests/test_regress_gpu.py to use the
restatements as its reference.

Limits: the goldens are fp32 results of sums of at most 48 terms, so 2e-6 relative per element for depths and samples (a few
ulp), 2e-6 absolute for confidences and weights (values in 0 .. 1); the spread goes through a square root of a difference of
depths and keeps the 2e-4 * max of tests/test_parity_gpu.py.
"""
import numpy as np
import pytest
import torch

import regress_ref as R
from conftest import load_golden

REL = 2e-6      # depths, samples: per element, relative
ABS01 = 2e-6    # confidences, weights: per element, absolute


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def _abs(got, want):
    return float(np.abs(got - np.asarray(want, np.float64)).max())


def test_softargmin_goldens():
    g = load_golden("ops_regress")
    assert int(g["n_softargmin"]) == 6
    for i in range(6):
        k = "sa%d_" % i
        r = R.softargmin(g[k + "cost"], g[k + "depth_values"])
        assert _rel(r.depth, g[k + "depth"]) <= REL, i
        assert _abs(r.conf, g[k + "conf"]) <= ABS01, i


def test_softargmin_variance_golden():
    g = load_golden("ops_ucsnet")
    r = R.softargmin(g["cd_pre"], g["cd_samps"], lamb=1.5)
    assert _rel(r.depth, g["cd_depth"]) <= REL
    assert _abs(r.var, g["cd_variance"]) <= 2e-4 * float(np.abs(g["cd_variance"]).max())


def test_online_regression_goldens():
    g = load_golden("ops_regress")
    assert int(g["n_online"]) == 3
    for i in range(3):
        k = "on%d_" % i
        reg, dpl = g[k + "reg"], g[k + "dplanes"]
        assert (dpl.shape != reg.shape) == bool(g[k + "up"])
        state = R.online_start(*reg.shape[1:])
        for d in range(reg.shape[0]):
            state = R.online_update(state, reg[d], dpl[d])
        dep, conf = R.online_finalize(state)
        assert _rel(dep, g[k + "depth"]) <= REL, i
        assert _abs(conf, g[k + "conf"]) <= ABS01, i
        # the resampled planes the reference accumulated are the restatement's
        if bool(g[k + "up"]):
            assert _rel(R.resize_bilinear(dpl, *reg.shape[1:]), g[k + "dplanes_up"]) <= REL, i


def test_depth_range_goldens():
    g = load_golden("ops_regress")
    D = g["dr0_out"].shape[0]
    want = g["dr0_out"]
    assert (want == want[:, :1, :1]).all()     # the reference tiles the planes over the map
    assert _rel(R.depth_range_plane(g["dr0_cur"], D), want[:, 0, 0]) <= REL
    D = g["dr1_out"].shape[0]
    assert _rel(R.depth_range_pixel(g["dr1_cur"], D, g["dr1_interval"]), g["dr1_out"]) <= REL
    lo, step = R.depth_range_maps(g["dr1_cur"], D, g["dr1_interval"])
    assert _rel(R.depth_planes((lo, step, D), *lo.shape), g["dr1_out"]) <= REL


def test_uncertainty_samples_goldens():
    g = load_golden("ops_ucsnet")
    want = g["s1_samples"]
    assert (want == want[:, :1, :1]).all()
    assert _rel(R.depth_range_plane(g["s1_depth_values"], want.shape[0]), want[:, 0, 0]) <= REL
    want = g["s2_samples"]
    assert _rel(R.uncertainty_samples(g["s2_cur"], g["s2_var"], want.shape[0]), want) <= REL


def test_pair_softmax_max_golden():
    g = load_golden("ops_pairnet")
    vw, pd = R.pair_softmax_max(g["score"], g["depth_values"])
    assert _abs(vw, g["view_weight"]) <= ABS01
    assert _rel(pd, g["pair_depth"]) <= REL


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_resize_bilinear_is_atens(case):
    """Against torch.nn.functional.interpolate in fp32 on the CPU, within 2 ulp of the value: ATen's blend is four fp32 products
    and three fp32 sums of positive terms, the restatement's is float64 on the same fp32 coordinates and weights."""
    h, w, H, W = case
    x = np.random.default_rng(h * 1000 + W).uniform(400, 800, (3, h, w)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    got = R.resize_bilinear(x, H, W)
    assert got.shape == want.shape and got.dtype == np.float64
    ulps = np.abs(got - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    assert ulps.max() <= 2.0, float(ulps.max())
    if (h, w) == (H, W):
        assert np.array_equal(got, x.astype(np.float64))


@pytest.mark.parametrize("mode", ["plane", "pixel", "affine"])
def test_softargmin_single_plane_and_one_hot_columns(mode):
    rng = np.random.default_rng(3)
    h, w = 5, 7

    def depths(D):
        if mode == "plane":
            return np.sort(rng.uniform(400, 800, D)).astype(np.float32)
        if mode == "pixel":
            return np.sort(rng.uniform(400, 800, (D, h, w)), 0).astype(np.float32)
        return (rng.uniform(400, 600, (h, w)).astype(np.float32), rng.uniform(0.5, 3, (h, w)).astype(np.float32), D)

    # D = 1: the only plane's depth, confidence 1, no spread
    dv = depths(1)
    r = R.softargmin(rng.standard_normal((1, h, w)), dv, lamb=1.5)
    assert np.array_equal(r.depth, R.depth_planes(dv, h, w)[0])
    assert np.array_equal(r.conf, np.ones((h, w))) and np.array_equal(r.index, np.zeros((h, w)))
    assert np.array_equal(r.var, np.zeros((h, w)))
    # a one-hot column at the first / the last plane: that plane's depth, confidence 1
    for D in (2, 3, 9):
        dv = depths(D)
        planes = R.depth_planes(dv, h, w)
        for k in (0, D - 1):
            cost = np.full((D, h, w), -np.inf)
            cost[k] = rng.standard_normal((h, w))
            r = R.softargmin(cost, dv, lamb=1.5)
            assert np.array_equal(r.depth, planes[k]) and np.array_equal(r.index, np.full((h, w), float(k)))
            assert np.array_equal(r.conf, np.ones((h, w)))
            assert np.array_equal(r.var, np.zeros((h, w)))
            assert np.array_equal(r.conf_at(k), r.conf) and np.array_equal(r.conf_at(k - 1 if k else k + 1), r.conf)


def test_affine_planes_are_the_fp32_volume():
    """(lo, step, D): plane k is fl(lo + fl(k * step)) in fp32 -- what the reference's [D,h,w] volume holds (module.py:625-628)."""
    rng = np.random.default_rng(4)
    lo = rng.uniform(400, 600, (6, 5)).astype(np.float32)
    step = rng.uniform(0.5, 3, (6, 5)).astype(np.float32)
    want = torch.from_numpy(lo)[None] + torch.arange(33, dtype=torch.float32).reshape(-1, 1, 1) * torch.from_numpy(step)[None]
    assert np.array_equal(R.depth_planes((lo, step, 33), 6, 5), want.numpy().astype(np.float64))
