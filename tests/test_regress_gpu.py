"""The kernels between the cost volume and the depth map (csrc/regress.hip: soft-argmin with and without the spread, pair softmax,
the two hypothesis samplers, bilinear resize, online regression) against the float64 restatements of tests/regress_ref.py, on
every dispatch path: the register-cached soft-argmin for DC = 8 / 16 / 32 / 48 / 64, the streaming one with 16-byte and with scalar
accesses, the three depth modes, the quad and the scalar form of each sampler, more than one workgroup, ragged last workgroups, and
inputs that are a multiple of four pixels but do not start on a 16-byte boundary.  All calls go through deep3d_aerial_amd.ops.
No pixel is left out of any assertion.

Errors.  An fp32 emulation of the kernels' arithmetic on the CPU (plane-order fmaf sums, fp32 exp, IEEE divide; every D and plane
below, both cost kinds and costs scaled by 40) against the restatement gave
    depth 2.8e-7 rel_l1 and 1.9e-6 relative per pixel, confidence 1.1e-6, spread 3.3e-6 * max;
the worst seen on an MI355X over every case of this file (the `ops` fixture prints them at the end of a run, pytest -s):
    depth 2.2e-7 rel_l1 and 1.2e-6 relative per pixel, confidence 1.3e-6, spread 2.5e-6 * max;
    pair softmax: view weight 7.9e-7, depth 8.6e-7 relative per pixel;
    uncertainty samples 5.9e-5, depth range samples 5.9e-5, resize 1.2e-4 (all absolute, on depths of 400 .. 800);
    online regression: accumulators and depth 2.7e-7 relative per pixel, confidence 1.3e-7.
The limits below are the project's constants (tests/test_parity_gpu.py) and leave the emulation 5 x or more; what the device adds
is its fast exponential.

What this file found: the resize kernel rounded the product of its source coordinate on its own where ATen fuses it into the
subtraction; at 17 x 23 -> 29 x 40 that put output row 27 and column 28 3.4e-4 from the restatement (limit 2.5e-4).  The resize
kernel now rounds once (csrc/regress.hip, lin_coord<true>); the online regression's resample keeps its two roundings, which its
depth tolerance does not see (2.7e-7 relative at 5 x 8 -> 13 x 131).

That the tests catch a wrong kernel was checked on the device with one arithmetic-only change at a time: the streaming kernel's
window cut to three planes fails D = 65 / 96 / 130 of test_softargmin_every_variant, the cached kernel's window cut to three fails
every D from 3 to 64 (D = 1 and 2 have no plane k + 2), the streaming kernel's max taken from the quad's first pixel fails the
"sharp" costs on 16 x 68 (elsewhere a wrong shift cancels in the softmax until it overflows), the resize kernel's plane loop
stepping by twice the grid fails n = 65 and 130 -- and serving D = 33 .. 48 from the 64-plane instance changes nothing, as it must.
"""
import functools

import numpy as np
import pytest
import torch

import regress_ref as R
from conftest import rel_l1

pytestmark = pytest.mark.gpu

REL_DEPTH = 1e-5      # depth maps: relative L1 of the map AND |got - ref| <= 1e-5 |ref| at every pixel (the second catches a bad tail)
ABS_CONF = 1e-5       # confidences and view weights (values in 0 .. 1), per pixel
REL_VAR = 2e-4        # spread: per pixel, times max(ref)
ABS_UNC = 1e-4        # uncertainty_aware_samples with spreads in 0 .. 20: three fp32 roundings, at 800 at most ~1.2 ulp = 7e-5
ABS_SAMPLES = 2.5e-4  # depth_range_samples, resize_bilinear
LAMB = 1.5

PLANES = [(7, 9),     # 63 pixels: under one workgroup, scalar path
          (12, 20),   # 240: quad path, one partial workgroup
          (33, 31),   # 1023: scalar path, ragged fourth workgroup
          (16, 68)]   # 1088 = 272 quads: quad path, ragged second workgroup
# (h, w, misaligned): the last one is 12 x 20 with every input one float into a larger buffer -- a multiple of four pixels that
# must take the scalar kernels
VARIANTS = [(h, w, False) for h, w in PLANES] + [(12, 20, True)]

WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deep3d_aerial_amd import _lib, ops as _ops

    _lib.load()  # raises if the HIP library is missing: no silent fallback
    yield _ops
    print("\nworst device errors: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def dev(a, misaligned=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()   # (a copy: the shared inputs are read-only)
    if not misaligned:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 7, dtype=torch.float32, device="cuda")
    view = buf[1:1 + t.numel()].view(t.shape)     # contiguous, 4 bytes past a 16-byte boundary (the view keeps `buf` alive)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def host(t):
    return t.detach().cpu().numpy()


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cost_volume(kind, D, h, w):
    """"noise": 3 N(0,1); "sharp": 40 N(0,1) (nearly one-hot columns, terms underflow); "peaked": the noise with one plane per
    pixel raised to max + 12 -- a random plane, but plane 0 along the top row and plane D-1 along the bottom row."""
    rng = np.random.default_rng([11, D, h, w])
    c = rng.standard_normal((D, h, w))
    if kind == "sharp":
        return _frozen(40 * c)
    c = 3 * c
    if kind == "peaked":
        k = rng.integers(0, D, (h, w))
        k[0], k[-1] = 0, D - 1
        np.put_along_axis(c, k[None], c.max(0, keepdims=True) + 12, 0)
    else:
        assert kind == "noise"
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def depth_vector(D):
    return _frozen(np.sort(np.random.default_rng([12, D]).uniform(400, 800, D)))


@functools.lru_cache(maxsize=None)
def depth_volume(D, h, w):
    return _frozen(np.sort(np.random.default_rng([13, D, h, w]).uniform(400, 800, (D, h, w)), 0))


@functools.lru_cache(maxsize=None)
def depth_maps(D, h, w):
    """(lo, step): plane k at lo + k * step stays in 400 .. 800."""
    rng = np.random.default_rng([14, D, h, w])
    return _frozen(rng.uniform(400, 600, (h, w))), _frozen(rng.uniform(20, 200, (h, w)) / max(D - 1, 1))


def run_softargmin(ops, cost, depth, lamb):
    if lamb is None:
        return ops.softargmin_conf4(cost, depth)
    return ops.softargmin_conf4_var(cost, depth, lamb)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def check_depth(got, ref, what="depth"):
    got = np.asarray(got, np.float64)
    l1, px = rel_l1(got, ref), float((np.abs(got - ref) / np.abs(ref)).max())
    note(what + " rel_l1", l1)
    note(what + " rel/pixel", px)
    assert l1 <= REL_DEPTH and px <= REL_DEPTH, (what, l1, px)


def check_softargmin(got, ref, tag):
    check_depth(host(got[0]), ref.depth)
    # The reference truncates the expected index.  Where the float64 index lies within 1e-3 of an integer n an fp32 index may
    # fall on either side: the window of n - 1 or of n; everywhere else the window of floor(index).
    conf = host(got[1]).astype(np.float64)
    n = np.rint(ref.index).astype(np.int64)
    near = np.abs(ref.index - n) <= 1e-3
    either = np.minimum(np.abs(conf - ref.conf_at(n - 1)), np.abs(conf - ref.conf_at(n)))
    err = np.where(near, either, np.abs(conf - ref.conf_at(np.floor(ref.index).astype(np.int64))))
    note("confidence", err.max())
    assert err.max() <= ABS_CONF, (tag, float(err.max()))
    if ref.var is not None:
        verr = np.abs(host(got[2]) - ref.var).max()
        if ref.var.max() > 0:
            note("spread / max", verr / ref.var.max())
        assert verr <= REL_VAR * ref.var.max(), (tag, float(verr), float(ref.var.max()))


# ----------------------------------------------------------------------------------------
# soft-argmin
# ----------------------------------------------------------------------------------------
# D <= 8 | 16 | 32 | 48 | 64: the register-cached kernel of that size, at its upper edge and one past it; 1, 2, 3: the four-plane
# window clipped on both sides; 65, 96, 130: the streaming kernel (quads on 12 x 20 and 16 x 68, scalars on the other planes and
# on the misaligned one)
@pytest.mark.parametrize("with_var", [False, True], ids=["conf4", "conf4_var"])
@pytest.mark.parametrize("D", [1, 2, 3, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 130])
def test_softargmin_every_variant(ops, D, with_var):
    lamb = LAMB if with_var else None
    for h, w, mis in VARIANTS:
        kinds = ["noise", "peaked"] + (["sharp"] if (h, w) in ((33, 31), (16, 68)) else [])
        for kind in kinds:
            tag = (D, h, w, mis, kind)
            c = cost_volume(kind, D, h, w)
            ct = dev(c, mis)
            # per plane [D], and the same floats as a [D,h,w] volume
            dv = depth_vector(D)
            got = run_softargmin(ops, ct, dev(dv, mis), lamb)
            assert same(got, run_softargmin(ops, ct, dev(np.broadcast_to(dv[:, None, None], (D, h, w)), mis), lamb)), tag
            check_softargmin(got, R.softargmin(c, dv, lamb), tag + ("plane",))
            # per pixel [D,h,w]
            dvol = depth_volume(D, h, w)
            check_softargmin(run_softargmin(ops, ct, dev(dvol, mis), lamb), R.softargmin(c, dvol, lamb), tag + ("pixel",))
            # affine maps, and the volume they stand for
            lo, step = depth_maps(D, h, w)
            aff = ops.AffineDepth(dev(np.stack([lo, step]), mis), D)
            vol = aff.volume()
            assert np.array_equal(host(vol), R.depth_planes((lo, step, D), h, w)), tag
            got = run_softargmin(ops, ct, aff, lamb)
            assert same(got, run_softargmin(ops, ct, vol, lamb)), tag
            check_softargmin(got, R.softargmin(c, (lo, step, D), lamb), tag + ("affine",))


@pytest.mark.parametrize("D", [8, 16, 32, 48, 64, 65])
def test_a_trailing_minus_inf_plane_changes_nothing(ops, D):
    """exp(-inf) = 0 adds exactly nothing to a plane-order fmaf sum (no fast-math, no contraction), so a (D+1)-plane call whose last
    plane costs -inf returns the D-plane call's floats.  D at a cached kernel's upper edge puts the two calls on different
    instances -- DC against the next DC, DC = 64 against the streaming kernel (quads on 16 x 68, scalars on 33 x 31), 65 the
    streaming kernel against itself -- which csrc/regress.hip promises to be the same arithmetic."""
    for h, w in ((16, 68), (33, 31)):
        last = np.full((1, h, w), 900.0, np.float32)
        lo, step = depth_maps(D, h, w)
        maps = dev(np.stack([lo, step]))
        depths = [(dev(depth_vector(D)), dev(np.append(depth_vector(D), np.float32(900.0)))),
                  (dev(depth_volume(D, h, w)), dev(np.concatenate([depth_volume(D, h, w), last]))),
                  (ops.AffineDepth(maps, D), ops.AffineDepth(maps, D + 1))]
        for kind in ("noise", "peaked"):
            c = cost_volume(kind, D, h, w)
            ct, ct1 = dev(c), dev(np.concatenate([c, np.full((1, h, w), -np.inf, np.float32)]))
            for mode, (d0, d1) in zip(("plane", "pixel", "affine"), depths):
                for lamb in (None, LAMB):
                    assert same(run_softargmin(ops, ct, d0, lamb), run_softargmin(ops, ct1, d1, lamb)), (D, h, w, kind, mode, lamb)


# ----------------------------------------------------------------------------------------
# pair softmax
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 5, 48, 70])
def test_pair_softmax_max_both_depth_modes(ops, D):
    for h, w in ((7, 9), (33, 31)):
        for kind in ("noise", "peaked"):
            s = cost_volume(kind, D, h, w)
            for dv in (depth_vector(D), depth_volume(D, h, w)):
                vw, pd = ops.pair_softmax_max(dev(s), dev(dv))
                rvw, rpd = R.pair_softmax_max(s, dv)
                err = np.abs(host(vw) - rvw).max()
                note("view weight", err)
                assert err <= ABS_CONF, (D, h, w, kind, dv.ndim)
                check_depth(host(pd), rpd, "pair depth")
        lo, step = depth_maps(D, h, w)
        with pytest.raises(TypeError):
            ops.pair_softmax_max(dev(s), ops.AffineDepth(dev(np.stack([lo, step])), D))


# ----------------------------------------------------------------------------------------
# hypothesis samplers
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 8, 33])
def test_uncertainty_samples_scalar_and_quad_paths(ops, D):
    for h, w, mis in VARIANTS:
        rng = np.random.default_rng([15, D, h, w])
        cur = rng.uniform(400, 800, (h, w)).astype(np.float32)
        var = rng.uniform(0, 20, (h, w)).astype(np.float32)
        var[1:5, 2:8] = 0.0           # no spread: every hypothesis is fl(cur + 1e-12) = cur
        ct, vt = dev(cur, mis), dev(var, mis)
        out = ops.uncertainty_aware_samples(ct, vt, D)
        got = host(out)
        assert got.shape == (D, h, w)
        err = np.abs(got - R.uncertainty_samples(cur, var, D)).max()
        note("uncertainty samples", err)
        assert err <= ABS_UNC, (D, h, w, mis, float(err))
        assert np.array_equal(got[:, 1:5, 2:8], np.broadcast_to(cur[1:5, 2:8], (D, 4, 6))), (D, h, w, mis)
        aff = ops.uncertainty_aware_samples(ct, vt, D, affine=True)
        assert aff.D == D and torch.equal(aff.volume(), out), (D, h, w, mis)


def test_depth_range_samples_every_form(ops):
    # per plane: one workgroup serves 64 planes, the second starts at D = 65
    mm = np.random.default_rng(16).uniform([400, 700], [500, 800]).astype(np.float32)
    for D in (2, 64, 65, 200):
        got = host(ops.depth_range_samples(dev(mm), D, 0.0))
        assert got.shape == (D,)
        err = np.abs(got - R.depth_range_plane(mm, D)).max()
        note("depth range samples", err)
        assert err <= ABS_SAMPLES, (D, float(err))
        assert got[0] == mm[0]
    # per pixel, and the two maps that generate the same planes
    interval = np.float32(2.6041665)
    for D in (2, 8, 48):
        for h, w, mis in VARIANTS:
            cur = np.random.default_rng([17, D, h, w]).uniform(400, 800, (h, w)).astype(np.float32)
            ct = dev(cur, mis)
            out = ops.depth_range_samples(ct, D, interval)
            assert tuple(out.shape) == (D, h, w)
            err = np.abs(host(out) - R.depth_range_pixel(cur, D, interval)).max()
            note("depth range samples", err)
            assert err <= ABS_SAMPLES, (D, h, w, mis, float(err))
            aff = ops.depth_range_affine(ct, D, interval)
            assert aff.D == D and torch.equal(aff.volume(), out), (D, h, w, mis)
            lo, step = R.depth_range_maps(cur, D, interval)
            assert np.abs(host(aff.maps) - np.stack([lo, step])).max() <= ABS_SAMPLES, (D, h, w, mis)


# ----------------------------------------------------------------------------------------
# bilinear resize
# ----------------------------------------------------------------------------------------
# n = 65 and 130: the grid holds 64 planes, a workgroup walks on to plane z + 64 (and z + 128).  At n = 3: non-integer ratio with
# quad stores, down-sampling, the identity, 65 quads (a second workgroup along x), scalar stores with a second workgroup along x and
# H no multiple of 4, and the two degenerate sizes (regress_ref.RESIZE_CASES)
RESIZE = [(n,) + R.RESIZE_CASES[0] for n in (1, 3, 64, 65, 130)] + [(3,) + c for c in R.RESIZE_CASES[1:]]


@pytest.mark.parametrize("case", RESIZE, ids=lambda c: "n%d-%dx%d-%dx%d" % c)
def test_resize_bilinear_grid_and_plane_loop(ops, case):
    n, h, w, H, W = case
    x = np.random.default_rng([18, n, h, w]).uniform(400, 800, (n, h, w)).astype(np.float32)
    xt = dev(x)
    out = ops.resize_bilinear(xt, H, W)
    assert tuple(out.shape) == (n, H, W)
    err = np.abs(host(out) - R.resize_bilinear(x, H, W)).max()
    note("resize", err)
    assert err <= ABS_SAMPLES, float(err)
    if (h, w) == (H, W):
        assert torch.equal(out, xt)


# ----------------------------------------------------------------------------------------
# online regression
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(9, 70), (13, 131), (4, 64)])
def test_online_regression_ragged_and_resampled(ops, H, W):
    """Five planes accumulated and finalised, with the depth plane at the map's resolution, at a smaller one in no integer ratio
    and as [1,1]; the three accumulators are compared one by one after the first update, so an error the finalising division
    cancels still shows."""
    nplanes = 5
    for hd, wd in ((H, W), (5, 8), (1, 1)):
        rng = np.random.default_rng([19, H, W, hd, wd])
        reg = rng.standard_normal((nplanes, H, W)).astype(np.float32)
        dpl = rng.uniform(400, 800, (nplanes, hd, wd)).astype(np.float32)
        acc = [torch.zeros(H, W, device="cuda") for _ in range(3)]
        state = R.online_start(H, W)
        for d in range(nplanes):
            ops.online_regress_update(dev(reg[d]), dev(dpl[d]), *acc)
            state = R.online_update(state, reg[d], dpl[d])
            if d == 0:
                for name, a, r in zip(("max_p", "sum_d", "sum_p"), acc, state):
                    check_depth(host(a), r, "online " + name)
        dep, conf = ops.online_regress_finalize(*acc)
        rdep, rconf = R.online_finalize(state)
        check_depth(host(dep), rdep, "online depth")
        err = np.abs(host(conf) - rconf).max()
        note("online confidence", err)
        assert err <= ABS_CONF, (H, W, hd, wd, float(err))
