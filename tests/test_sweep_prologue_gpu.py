"""The ring kernel's planning prologue (csrc/planesweep_tiled.hip: one wave per source view plans that view's windows, ring and
delta rectangles) at the smallest shapes at which a plan can still go wrong, against the float64 restatement of tests/sweep_ref.py
with test_sweep_views_gpu's bounds.  Every case forces the ring family and asserts from the library's counters that it served.

  patch width     w % 32 in {0, 1, 16, 17, 31}: wide and tall last patch columns
  patch height    h % 4 != 0 and h % 8 != 0 (the tall patches are 8 rows high)
  step sizes      D in {1, 5, 17, 33}: one step, a ragged last step, the candidates of 16 / 8 / 4 planes
  segments        D = 130: two depth segments, the second one two planes long
  view counts     V = 2 .. 7: the two-, four- and six-source templates, full and with an unused slot
  channels        one and two 16-channel passes; 8-channel groups on the shallow form (32 x 8 patches)
  hypotheses      per plane, affine and per pixel
  half step       plane spacing so wide that only the half-step candidate's rings fit
  gather          a source view behind every plane (p.z < 0 at the patch corners): the workgroups gather from global memory
"""
import functools

import numpy as np
import pytest

import sweep_ref as R
from test_sweep_views_gpu import ABS_GATHER, REL_VOLUME, _depth_dev, _held, _run, dev, host, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

assert ABS_GATHER == 1e-3 and REL_VOLUME == 5e-5

# V, C, h, w, D, hypotheses, sweep in pixels (None: D / 2)
CASES = {
    # patch width (h = 9: the last patch row is one pixel high)
    "w64": (3, 16, 9, 64, 5, "plane", None),
    "w33_tall": (3, 16, 9, 33, 5, "plane", None),
    "w48_tall": (3, 16, 9, 48, 5, "plane", None),
    "w49": (3, 16, 9, 49, 5, "plane", None),
    "w63": (3, 16, 9, 63, 5, "plane", None),
    # patch height: h % 8 = 6 and 4 below a tall column (8-row patches), h % 4 = 2 and 3 below a wide one
    "h6_tall": (3, 16, 6, 48, 5, "plane", None),
    "h12_tall": (3, 16, 12, 40, 5, "plane", None),
    "h6_wide": (3, 16, 6, 63, 5, "plane", None),
    "h11_wide": (3, 16, 11, 32, 5, "plane", None),
    # step sizes
    "D1": (3, 16, 9, 33, 1, "affine", None),       # (one plane has no spacing to derive per-plane depths from)
    "D1_pixel": (3, 16, 9, 33, 1, "pixel", None),
    "D17": (3, 16, 9, 33, 17, "plane", None),
    "D33": (3, 16, 9, 33, 33, "plane", None),
    "D33_wide_sweep": (3, 16, 9, 49, 33, "plane", 40.0),
    # two segments
    "D130": (4, 16, 9, 33, 130, "plane", 6.0),
    # view counts (V - 1 sources)
    "V2": (2, 16, 9, 49, 5, "plane", None),
    "V4": (4, 16, 9, 49, 5, "plane", None),
    "V5": (5, 16, 9, 49, 5, "plane", None),
    "V6": (6, 16, 9, 49, 5, "plane", None),
    "V7": (7, 16, 9, 49, 18, "plane", None),
    # channels: two passes; 8-channel groups (shallow form up to 16 planes, deep form beyond)
    "C32": (5, 32, 9, 49, 17, "plane", None),
    "C8_shallow": (5, 8, 13, 49, 8, "plane", None),
    "C8_deep": (3, 8, 9, 33, 17, "plane", None),
    # hypothesis forms
    "affine": (5, 16, 9, 49, 17, "affine", None),
    "pixel": (5, 16, 9, 49, 17, "pixel", None),
    "affine_shallow": (5, 8, 13, 48, 8, "affine", None),
    "pixel_two_passes": (3, 32, 6, 33, 5, "pixel", None),
}
# Half step.  Four sources share the LDS (about 9 k floats of ring each), rolled by yaws of about 10 degrees, so that a 225-pixel-wide
# window row climbs some 40 source rows; 20 planes and 90 px of disparity across them.  A ring must hold two consecutive windows
# (16 / 8 / 4 planes per step: 32 / 16 / 8 planes' worth of disparity); restating the planner's fit test (corner hull of every
# step, union of neighbours, ring pitch) on the CPU gives 15 of the 23 workgroups the half step of 2 planes, 6 the 4-plane step
# and the two at the image's ends the 16-plane step; none gathers.
HALF_STEP = (5, 16, 9, 225, 20, "plane", 90.0, 10.0)

for _name, _c in list(CASES.items()) + [("half_step", HALF_STEP)]:
    assert R.f32_tiled(_c[0], _c[1]), _name       # inside the ring family's domain: no case can be refused or skipped


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Scene, composed projections on the device and the float64 variance volume of a case: computed once, never written to."""
    from deep3d_aerial_amd import ops as _ops

    V, C, h, w, D, kind, sweep = case[:7]
    sc = R.Scene(V, C, h, w, D, kind, sweep_px=sweep, **({"yaw_deg": case[7]} if len(case) > 7 else {}))
    p34 = _ops.compose_projections(dev(sc.proj))
    return sc, p34, R.variance_volume(sc.feats, host(p34).reshape(-1, 3, 4), sc.depth)


@pytest.mark.parametrize("name", list(CASES))
def test_ring_plan(ops, name):
    sc, p34, want = _inputs(CASES[name])
    fd = [dev(f) for f in sc.feats]
    depth, _ = _depth_dev(ops, sc.depth)
    got = _run(ops, "tiled", lambda: ops.variance_volume(fd, p34, depth))
    _held("variance", host(got), want)


@pytest.mark.parametrize("name", ["V4", "affine", "C8_shallow"])
def test_ring_plan_weighted(ops, name):
    """The visibility-weighted mode shares the prologue (another instantiation of the kernel)."""
    sc, p34, _ = _inputs(CASES[name])
    fd, vw = [dev(f) for f in sc.feats], dev(sc.weights)
    depth, _ = _depth_dev(ops, sc.depth)
    got = _run(ops, "tiled", lambda: ops.weighted_corr(fd, p34, vw, depth))
    _held("weighted", host(got), R.weighted_corr(sc.feats, host(p34).reshape(-1, 3, 4), sc.weights, sc.depth))


def test_half_step_candidate(ops):
    sc, p34, want = _inputs(HALF_STEP)
    fd, depth = [dev(f) for f in sc.feats], dev(sc.depth)
    got = _run(ops, "tiled", lambda: ops.variance_volume(fd, p34, depth))      # (the ring family served: _run asserts it)
    _held("variance", host(got), want)


def test_gather_fallback_behind_the_plane(ops):
    """The last source lies behind every plane (p.z = -1) and projects 5000 px out of frame: no hull bounds its windows, every
    workgroup gathers its taps from global memory, and the view adds exact zeros -- as the restatement's does."""
    sc, p34, _ = _inputs(CASES["V4"])
    p34 = p34.clone()
    p34[-1] = dev(np.array([0, 0, 0, 5000, 0, 0, 0, 5000, 0, 0, 0, -1], np.float32)).reshape(p34[-1].shape)
    fd, depth = [dev(f) for f in sc.feats], dev(sc.depth)
    got = _run(ops, "tiled", lambda: ops.variance_volume(fd, p34, depth))
    _held("variance", host(got), R.variance_volume(sc.feats, host(p34).reshape(-1, 3, 4), sc.depth))
