"""The plane-sweep kernels at the view counts, channel widths and storage types the other suites never reach, against the float64
restatement of tests/sweep_ref.py (tests/test_sweep_ref.py ties that one to the reference's outputs, to ATen and to the C oracle).

  fp32    V = 6 (five sources on the six-source ring templates, an empty slot; 8-channel groups), V = 8, 9, 16 (past launch_tiled
          and launch_window: the direct kernel's view loop up to D3D_MAX_VIEWS), each on per-plane, per-pixel and affine hypotheses.
  fp16    launch_f16<2>, <4> and <6> with one to six sources, one to three channel groups, all three hypothesis forms, more than
          one depth segment; the direct kernel's fp16 instantiations <16 | 8 | 4 | 1, __half>, which serve every fp16 call that
          launch_f16 refuses (C % 16 != 0, more than six sources, no workspace).
  refusals, degenerate source views (p.z == 0, far out of frame) in the aggregation modes, calls without a workspace.

Bounds.  fp32: test_parity_gpu's, unchanged -- the C oracle is within 6e-5 max abs / 3e-6 relative L1 of the float64 restatement
on these cases (test_sweep_ref.py), a tenth of them.  fp16: half an ulp of the stored value on top of the fp32 bound, per voxel,
and the share of voxels whose stored value is not RNE16 of the float64 value is held to a cap taken from the same share of the C
oracle's fp32 output (see _check_fp16).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sweep_ref as R
from deep3d_aerial_amd import config

pytestmark = pytest.mark.gpu

ABS_GATHER = 1e-3     # max abs error of a warped N(0,1) white-noise feature (test_parity_gpu.ABS_GATHER)
REL_VOLUME = 5e-5     # relative L1 of a whole cost volume (test_parity_gpu.REL_VOLUME)
FAMILIES = ("direct", "tiled", "window")


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
    return torch.from_numpy(np.array(a, order="C")).cuda()    # (a copy: the shared host inputs are read-only; the dtype is kept)


def host(t):
    return t.detach().cpu().numpy()


def _run(ops, family, fn, serves=None):
    """fn() on the dispatcher's choice ("auto") or with one kernel family forced.  Asserts from the library's own counters that
    the family asked for -- on "auto": the family `serves` -- is the only one that ran."""
    config.switches["D3D_FORCE_PATH"] = "" if family == "auto" else family
    try:
        ops._sync_force_path()
        ops.sweep_dispatch_counts(reset=True)
        out = fn()
        counts = ops.sweep_dispatch_counts()
    finally:
        config.switches["D3D_FORCE_PATH"] = ""
    want = serves if family == "auto" else family
    if want is not None:
        assert counts[want] > 0 and all(n == 0 for k, n in counts.items() if k != want), (family, want, counts)
    return out


def _depth_dev(ops, depth):
    """(what the sweep takes, the same hypotheses as a [D,h,w] volume or None): affine hypotheses go in as AffineDepth."""
    if isinstance(depth, tuple):
        lo, step, D = depth
        aff = ops.AffineDepth(dev(np.stack([lo, step])), D)
        return aff, aff.volume()
    return dev(depth), None


def _held(name, got, want, abs_bound=2 * ABS_GATHER, rel_bound=REL_VOLUME):
    err, rel = float(np.abs(got - want).max()), R.rel_l1(got, want)
    print("%s vs float64: max abs %.3g, rel-L1 %.3g" % (name, err, rel))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= abs_bound, name
    assert rel_bound is None or rel <= rel_bound, name


# ----------------------------------------------------------------------------------------
# 3a. fp32: the missing view counts
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fp32_inputs(row, kind):
    """Device inputs and float64 references of a case, computed once and shared by the families (nothing writes to them)."""
    from deep3d_aerial_amd import ops

    sc = R.fp32_scene(row, kind)
    p34 = ops.compose_projections(dev(sc.proj))
    p34_host = host(p34).reshape(-1, 3, 4)         # the reference gets the composed fp32 matrices the kernels get
    return sc, p34, R.variance_volume(sc.feats, p34_host, sc.depth), R.weighted_corr(sc.feats, p34_host, sc.weights, sc.depth)


FP32_PARAMS = [pytest.param(f, r, k, id="%s-%s" % (f, R.fp32_id(r, k))) for r in R.FP32_ROWS for k in R.DEPTH_KINDS for f in r[5]]


@pytest.mark.parametrize("family,row,kind", FP32_PARAMS)
def test_fp32_view_counts(ops, family, row, kind):
    sc, p34, want_var, want_wc = _fp32_inputs(row, kind)
    fd, vw = [dev(f) for f in sc.feats], dev(sc.weights)
    depth, vol = _depth_dev(ops, sc.depth)
    # the dispatcher: the window kernel takes at most four sources, the ring kernel six and 8-channel groups, the direct kernel the rest
    serves = "tiled" if R.f32_tiled(sc.V, sc.C) else "direct"
    var, wc = _run(ops, family, lambda: (ops.variance_volume(fd, p34, depth), ops.weighted_corr(fd, p34, vw, depth)), serves)
    if vol is not None:
        assert np.array_equal(host(vol), sc.depth_f32())       # the maps stand for the volume the reference was given, bit for bit
        var_v, wc_v = _run(ops, family, lambda: (ops.variance_volume(fd, p34, vol), ops.weighted_corr(fd, p34, vw, vol)), serves)
        assert torch.equal(var, var_v) and torch.equal(wc, wc_v)
    _held("variance", host(var), want_var)
    _held("weighted", host(wc), want_wc)


# ----------------------------------------------------------------------------------------
# 3b. fp16 storage
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fp16_inputs(row):
    import oracle
    from deep3d_aerial_amd import ops

    oracle.build()
    sc = R.fp16_scene(row)
    p34 = ops.compose_projections(dev(sc.proj))
    p34_host = host(p34).reshape(-1, 3, 4)
    want = R.variance_volume(sc.feats, p34_host, sc.depth)                # the fp16 values, widened to float64
    f = sc.feats.astype(np.float32)
    want_oracle = oracle.variance_volume(f[0], f[1:], p34_host, sc.depth_f32())
    return sc, p34, want, want_oracle


def _check_fp16(name, got, want, want_oracle):
    """got: fp16 [C,D,h,w] from a kernel; want: float64; want_oracle: the C oracle's fp32 volume on the same values.
    (1) per voxel, half an fp16 ulp of the value on top of the fp32 bound;
    (2) the rounding: the share of voxels whose stored value is not RNE16(want).  An fp32 result rounds to another fp16 value than
        the exact one wherever it lies on the other side of a rounding boundary, so the share grows with the fp32 error: the C
        oracle (~6e-5 from exact) shows 0.27 % .. 2.1 % on these cases, and the kernels' documented coordinate rounding (v_rcp_f32, ~3e-4) puts
        them about five times further out -- the cap is eight times the oracle's share on the same values (at least 2 %).  A
        truncating or double-rounded store flips about half of all voxels.  Measured on an MI355X: 0.25 % .. 1.96 %, between
        0.83 and 0.96 of the oracle's share on every row (the kernels skip the oracle's normalise / un-normalise round trip)."""
    assert got.dtype == np.float16 and got.shape == want.shape
    g = got.astype(np.float64)
    assert np.isfinite(g).all()
    excess = np.abs(g - want) - (2.0 ** -11 * np.abs(want) + 2 * ABS_GATHER)
    rne = want.astype(np.float16)
    share = float(np.mean(got != rne))
    share_oracle = float(np.mean(want_oracle.astype(np.float16) != rne))
    print("%s vs float64: max abs %.3g, rel-L1 %.3g, worst excess over the voxel bound %.3g; not RNE16: %.3f %% (oracle %.3f %%, ratio %.2f)"
          % (name, np.abs(g - want).max(), R.rel_l1(g, want), excess.max(), 100 * share, 100 * share_oracle, share / max(share_oracle, 1e-9)))
    assert excess.max() <= 0.0, name
    assert share <= max(8 * share_oracle, 0.02), name


def _fp16_families(V, C):
    return ("auto", "tiled", "direct") if R.f16_tiled(V, C) else ("auto", "direct")


FP16_PARAMS = [pytest.param(f, r, id="%s-%s" % (f, R.fp16_id(r))) for r in R.FP16_ROWS for f in _fp16_families(r[0], r[1])]


@pytest.mark.parametrize("family,row", FP16_PARAMS)
def test_fp16_storage(ops, family, row):
    sc, p34, want, want_oracle = _fp16_inputs(row)
    fd = [dev(f) for f in sc.feats]
    assert fd[0].dtype == torch.float16
    depth, vol = _depth_dev(ops, sc.depth)
    serves = "tiled" if R.f16_tiled(sc.V, sc.C) else "direct"       # the fall-through rows must count `direct`
    got = _run(ops, family, lambda: ops.variance_volume(fd, p34, depth), serves)
    assert got.dtype == torch.float16 and tuple(got.shape) == (sc.C, sc.D, sc.h, sc.w)
    _check_fp16("fp16 variance", host(got), want, want_oracle)
    if family == "direct":
        # one template, ldf / stf apart: the fp32 direct kernel on the same values, rounded once
        f32 = _run(ops, "direct", lambda: ops.variance_volume([f.float() for f in fd], p34, depth))
        print("fp16 direct vs RNE16(fp32 direct): %d voxels differ" % int((got != f32.half()).sum()))
        assert torch.equal(got, f32.half())
    if vol is not None:
        assert np.array_equal(host(vol), sc.depth_f32())
        assert torch.equal(got, _run(ops, family, lambda: ops.variance_volume(fd, p34, vol), serves))


# ----------------------------------------------------------------------------------------
# 3c. refusals
# ----------------------------------------------------------------------------------------
def _small(ops, V, C, half):
    sc = R.Scene(V, C, 12, 40, 3, "plane", half=half)
    return [dev(f) for f in sc.feats], ops.compose_projections(dev(sc.proj)), dev(sc.depth), dev(sc.weights)


@pytest.mark.parametrize("family,V,C,half", [("tiled", 3, 8, True), ("tiled", 8, 16, False), ("tiled", 8, 16, True), ("window", 6, 16, False),
                                             ("window", 3, 16, True), ("window", 6, 32, True)],
                         ids=lambda v: str(v))
def test_a_forced_family_refuses_what_is_outside_its_domain(ops, family, V, C, half):
    """A forced family raises on a shape it has no kernel for -- it neither computes something nor hands the call on -- and the
    dispatch counters stay where they were."""
    fd, p34, depth, vw = _small(ops, V, C, half)
    out = torch.full((C, 3, 12, 40), 7.0, dtype=fd[0].dtype, device="cuda")
    config.switches["D3D_FORCE_PATH"] = family
    ops._sync_force_path()
    ops.sweep_dispatch_counts(reset=True)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.variance_volume(fd, p34, depth, out=out)
    if not half:
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.weighted_corr(fd, p34, vw, depth)
    assert ops.sweep_dispatch_counts() == {"direct": 0, "tiled": 0, "window": 0}
    assert bool((out == 7.0).all())                       # nothing was launched on the output
    config.switches["D3D_FORCE_PATH"] = ""
    got = _run(ops, "auto", lambda: ops.variance_volume(fd, p34, depth))     # the dispatcher serves the same call
    assert bool(torch.isfinite(got.float()).all())


def test_fp16_argument_checks(ops):
    fd, p34, depth, _ = _small(ops, 3, 16, True)
    with pytest.raises(ValueError):
        ops.variance_volume(fd, p34, depth, plane_major=True)
    f32 = [f.float() for f in fd]
    ops.sweep_dispatch_counts(reset=True)
    with pytest.raises(TypeError):
        ops.variance_volume([fd[0], f32[1], fd[2]], p34, depth)
    with pytest.raises(TypeError):
        ops.variance_volume([f32[0], fd[1], f32[2]], p34, depth)
    assert ops.sweep_dispatch_counts() == {"direct": 0, "tiled": 0, "window": 0}


# ----------------------------------------------------------------------------------------
# 3d. degenerate source views in the aggregation modes
# ----------------------------------------------------------------------------------------
DEGENERATE = [pytest.param(8, False, id="C8_constant"), pytest.param(16, True, id="C16_noise")]


def _degenerate(C, noise):
    feats, wts = R.degenerate_feats(C, noise), R.degenerate_weights()
    return feats, wts, R.degenerate_closed_forms(feats, wts)


@pytest.mark.parametrize("C,noise", DEGENERATE)
@pytest.mark.parametrize("family", ("auto",) + FAMILIES)
def test_degenerate_views_add_exact_zeros(ops, family, C, noise):
    """One source with p.z == 0 (infinite / NaN coordinates), one 5000 px out of frame, one identity: the ring and window kernels
    plan their staging windows from the projected hull of exactly these views."""
    feats, wts, (variance, weighted, pair) = _degenerate(C, noise)
    fd, vw = [dev(f) for f in feats], dev(wts)
    p34, depth = dev(R.DEGENERATE_PROJ.reshape(3, 12)), dev(R.DEGENERATE_DEPTH)
    zeros = torch.zeros_like(fd[0])
    eye = p34[R.DEGENERATE_IDENTITY]
    # the same call with the dead views replaced by all-zero maps seen through the identity: what "adds exact zeros" means
    live = [fd[0]] + [fd[i + 1] if i == R.DEGENERATE_IDENTITY else zeros for i in range(3)]
    p34_live = torch.stack([eye, eye, eye]).contiguous()

    def sweep():
        return (ops.variance_volume(fd, p34, depth), ops.weighted_corr(fd, p34, vw, depth),
                torch.stack([ops.pair_corr_mean(fd[0], fd[i + 1], p34[i].contiguous(), depth) for i in range(3)]),
                ops.variance_volume(live, p34_live, depth), ops.weighted_corr(live, p34_live, vw, depth))

    var, wc, pm, var_live, wc_live = _run(ops, family, sweep)
    _held("variance", host(var), variance)
    _held("weighted", host(wc), weighted)
    _held("pair mean", host(pm), pair, ABS_GATHER, None)
    for i in range(3):
        if i != R.DEGENERATE_IDENTITY:
            assert int(torch.count_nonzero(pm[i])) == 0, i
    assert torch.equal(var, var_live) and torch.equal(wc, wc_live)
    _held("variance (restatement)", host(var), R.variance_volume(feats, R.DEGENERATE_PROJ, R.DEGENERATE_DEPTH))
    _held("weighted (restatement)", host(wc), R.weighted_corr(feats, R.DEGENERATE_PROJ, wts, R.DEGENERATE_DEPTH))


@pytest.mark.parametrize("family,C,noise", [("direct", 8, False), ("direct", 16, True), ("tiled", 16, True), ("auto", 16, True)])
def test_degenerate_views_fp16(ops, oracle, family, C, noise):
    feats, wts, _ = _degenerate(C, noise)
    f16 = feats.astype(np.float16)
    variance = R.degenerate_closed_forms(f16, wts)[0]
    fd = [dev(f) for f in f16]
    p34, depth = dev(R.DEGENERATE_PROJ.reshape(3, 12)), dev(R.DEGENERATE_DEPTH)
    got = _run(ops, family, lambda: ops.variance_volume(fd, p34, depth), "tiled")
    f32 = f16.astype(np.float32)
    _check_fp16("fp16 variance", host(got), variance, oracle.variance_volume(f32[0], f32[1:], R.DEGENERATE_PROJ, R.DEGENERATE_DEPTH))


# ----------------------------------------------------------------------------------------
# 3e. the workspace is optional
# ----------------------------------------------------------------------------------------
def _raw_variance(ops, fd, p34, depth, workspace):
    """d3d_variance_volume / d3d_variance_volume_f16 through the C ABI, with no workspace or with one of exactly the size the
    library asks for.  That one is the head of a block eight times as large whose every byte is 0xff (NaNs, as fp16 and as fp32):
    a kernel that reads past the size it was given -- the cells of a template slot without a view, say -- meets a NaN there
    instead of whatever the allocator left, and the read stays inside the block."""
    from deep3d_aerial_amd import _lib

    C, h, w = fd[0].shape
    V, D = len(fd), depth.shape[0]
    half = fd[0].dtype == torch.float16
    out = torch.empty((C, D, h, w), dtype=fd[0].dtype, device="cuda")
    arr = (ctypes.c_void_p * V)(*[f.data_ptr() for f in fd])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ops._sync_force_path()
    if workspace:
        n = int(_lib.load().d3d_sweep_workspace_bytes_for(V, C, D, h, w, 2 if half else 4, ops.PER_PLANE))
        assert n > 0
        buf = torch.full((8 * n,), 0xff, dtype=torch.uint8, device="cuda")
        wp, wn = ptr(buf), n
    else:
        wp, wn = ctypes.c_void_p(0), 0
    name = "d3d_variance_volume_f16" if half else "d3d_variance_volume"
    rc = getattr(_lib.load(), name)(arr, ptr(p34), ptr(depth), ops.PER_PLANE, V, C, D, h, w, ptr(out), wp, wn, ops._stream())
    _lib.check(rc, name)
    torch.cuda.synchronize()
    return out


def test_ring_kernel_without_a_workspace_reads_the_planar_maps(ops):
    """D >= 96 asks for the channel-last copy; without a workspace the ring kernel's planar loaders serve the same call, bit for bit."""
    sc = R.Scene(4, 16, 8, 16, 130, "plane", sweep_px=6.0)       # (three sources on the four-source template: one empty slot)
    fd, p34, depth = [dev(f) for f in sc.feats], ops.compose_projections(dev(sc.proj)), dev(sc.depth)
    with_ws = _run(ops, "tiled", lambda: _raw_variance(ops, fd, p34, depth, True))
    without = _run(ops, "tiled", lambda: _raw_variance(ops, fd, p34, depth, False))
    assert torch.equal(with_ws, _run(ops, "tiled", lambda: ops.variance_volume(fd, p34, depth)))
    print("planar loaders vs channel-last copy: %d voxels differ" % int((with_ws != without).sum()))
    assert torch.equal(with_ws, without)
    _held("variance", host(without), R.variance_volume(sc.feats, host(p34).reshape(-1, 3, 4), sc.depth))


def test_fp16_without_a_workspace_goes_to_the_direct_kernel(ops, oracle):
    """The fp16 ring loaders only read the channel-last copy: with no workspace the dispatcher hands the call to the direct kernel."""
    sc = R.Scene(5, 32, 21, 38, 6, "plane", half=True)
    fd, p34, depth = [dev(f) for f in sc.feats], ops.compose_projections(dev(sc.proj)), dev(sc.depth)
    got = _run(ops, "auto", lambda: _raw_variance(ops, fd, p34, depth, False), "direct")
    _run(ops, "auto", lambda: _raw_variance(ops, fd, p34, depth, True), "tiled")          # (with one, the ring kernel takes it)
    p34_host = host(p34).reshape(-1, 3, 4)
    f = sc.feats.astype(np.float32)
    _check_fp16("fp16 variance", host(got), R.variance_volume(sc.feats, p34_host, sc.depth), oracle.variance_volume(f[0], f[1:], p34_host, sc.depth))
    f32 = _run(ops, "direct", lambda: ops.variance_volume([x.float() for x in fd], p34, depth))
    assert torch.equal(got, f32.half())


@pytest.mark.parametrize("V,half,D", [(2, True, 3), (4, True, 3), (6, True, 3), (7, True, 3), (2, False, 100), (6, False, 100)],
                         ids=lambda v: str(v))
def test_ring_kernel_reads_nothing_past_its_workspace(ops, V, half, D):
    """The channel-last copy holds the views there are.  A template with more slots than views (NSRC = 2 | 4 | 6 for 1 .. 2 | 3 .. 4 |
    5 .. 6 sources) must not stage a cell of the missing ones from behind it: such a cell only ever meets weight 0, but 0 x NaN
    is a NaN in every voxel of the patch.  fp16 sweeps always use the copy, fp32 ones from 96 planes on."""
    sc = R.Scene(V, 16, 12, 40, D, "plane", sweep_px=4.0, half=half)
    fd, p34, depth = [dev(f) for f in sc.feats], ops.compose_projections(dev(sc.proj)), dev(sc.depth)
    got = host(_run(ops, "tiled", lambda: _raw_variance(ops, fd, p34, depth, True))).astype(np.float64)
    want = R.variance_volume(sc.feats, host(p34).reshape(-1, 3, 4), sc.depth)
    assert np.isfinite(got).all()
    excess = np.abs(got - want) - ((2.0 ** -11 * np.abs(want) if half else 0.0) + 2 * ABS_GATHER)
    print("max abs %.3g, worst excess over the voxel bound %.3g" % (np.abs(got - want).max(), excess.max()))
    assert excess.max() <= 0.0
