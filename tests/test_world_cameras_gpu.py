"""World-frame cameras on the device: the projection composition against exact rational arithmetic (tests/camera_ref.py), and the
sweeps, the warps and four whole models fed with cameras whose reference view is no longer K [I|0].

Every other suite builds its cameras with synthetic.make_scene, where ten of the sixteen entries of ref_proj are zero or one and
most of the 96 products of the cofactor expansion vanish.  Here every scene is moved by the rigid motions of
camera_ref.world_motions(): nadir-looking rotations, camera centres 0 .. 100 km from the origin, translation entries up to 1.8e8.

  a. ops.compose_projections, 16 motions x {make_scene at V = 2, 5, 16; the 688 x 464 frame at f = 1750 px} x stage scale {1, 0.25},
     per source view: every entry within one fp32 ulp of the exact entry, and the displacement over the whole frame at most twice
     that of RNE32(exact), plus 1e-7 px.  Measured on an MI355X over the 128 cases: worst entry 0.498 ulp, worst
     ratio to the displacement bound 0.499 (got 4.04e-5 px, ideal 4.04e-5 px, the aerial frame at scale 1) -- the kernel returns
     RNE32 of the exact value.  Its fp64 predecessor met the displacement bound and missed the ulp condition (1.7 ulp on the aerial
     frame under the general rotation, tests/test_camera_ref.py); the kernel now composes in double-double (csrc/compose_dd.h).
  b. d3d_compose_projections_f64 on float64 world-frame matrices that are no fp32 values: at most 16 times the displacement of
     numpy's float64 src @ inv(ref) from the exact result (floor 1e-12 px).  Measured, kernel / numpy, worst
     over the four rotations: make_scene 0 km 2.9e-14 / 3.1e-14, 1 km 8.2e-14 / 5.5e-14, 10 km 4.8e-13 / 8.0e-13, 100 km 1.3e-11 /
     8.2e-12 px; aerial frame 0 km 3.1e-13 / 2.5e-13, 1 km 1.6e-12 / 1.3e-12, 10 km 6.7e-12 / 7.4e-12, 100 km 1.1e-10 / 5.5e-11 px;
     the kernel is at most 3.0 times numpy on any case.
  c. the sweeps end to end: one row per kernel family (ring, direct, direct past the ring kernel, window, fp16 storage), moved by
     yaw90flip_10km and general_100km, against the float64 restatement reading the EXACT matrix -- not the kernel's p34 -- under
     test_sweep_views_gpu's bounds, unchanged (_held: 2e-3 max abs, 5e-5 rel-L1; _check_fp16).  Measured, max abs / rel-L1 (bounds 2e-3 /
     5e-5): ring and direct on FP32_ROWS[0] 3.9e-5 / 3.0e-6 variance, 4.8e-5 / 5.2e-6 weighted; direct on FP32_ROWS[3] 2.0e-5 /
     1.7e-6, 1.7e-5 / 3.1e-6; window 6.2e-5 / 3.0e-6, 6.6e-5 / 4.6e-6; fp16 storage (ring and direct alike) 0 voxels over the voxel
     bound, 0.69 % .. 0.71 % not RNE16 against the oracle's 0.78 % .. 0.83 % (cap: eight times the oracle's); the warps 6.4e-5
     (float) and 2.5e-5 (double) max abs against 1e-3.
  d. Infer_CascadeMVSNet, Infer_AdaMVSNet, Infer_CascadeREDNet and Infer_UCSNet with proj_stage1..3 moved by yaw90flip_10km against
     the goldens of the camera-frame inputs (a rigid motion of the world changes no output; tests/test_camera_ref.py holds the
     precondition), under the bounds of test_model_forward_matches_reference / test_ucsnet_forward_matches_reference, unchanged.
     Measured rel-L1, worst stage, moved / camera frame: casmvsnet_v3 depth 7.4e-7 / 1.8e-7, confidence 1.3e-5 / 2.7e-6;
     adamvs_v5 3.9e-7 / 1.9e-7, 8.2e-6 / 1.3e-6, view weights 4.1e-6 / 1.0e-6; msrednet_v3 8.4e-6 / 8.5e-7, 2.3e-4 / 2.4e-5 (bounds
     2e-5, 4e-4, 1e-3); ucsnet_v3 depth 4.6e-6 / 5.1e-7, confidence 2.7e-4 / 3.0e-6, variance 1.2e-5 / 1.3e-6 (bounds 1e-3, 5e-3,
     2e-2).  The moved errors are larger because moving rounds the stage matrices to fp32 again, which shifts the samples by up to
     1.9e-4 px (the precondition); no fixture is stepped down from 10 km.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import camera_ref as CR
import sweep_ref as R
from conftest import load_golden, rel_l1
from deep3d_aerial_amd import synthetic as S
from test_parity_gpu import REL_CONF_FP32, REL_MODEL, REL_MODEL_FP32, WINDOW_CASES, _fill
from test_sweep_views_gpu import ABS_GATHER, _check_fp16, _depth_dev, _held, _run, dev, host, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

MOTIONS = CR.world_motions()
SWEEP_MOTIONS = ("yaw90flip_10km", "general_100km")


def _exact34(proj):
    """[V,4,4] -> float64 [V-1,3,4]: the exact composition of every source view, each entry rounded once."""
    return np.stack([CR.exact_compose(proj[i], proj[0])[0] for i in range(1, proj.shape[0])])


# ----------------------------------------------------------------------------------------
# a. the fp32 composition
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.25], ids=["scale1", "scale0.25"])
@pytest.mark.parametrize("name", ["small_V2", "small_V5", "small_V16", "aerial"])
@pytest.mark.parametrize("m", MOTIONS, ids=lambda m: m.name)
def test_compose_projections_on_world_cameras(ops, m, name, scale):
    proj, h, w, depths = CR.scene(name, scale)
    moved = CR.move(proj, m.G)
    got = host(ops.compose_projections(dev(moved))).reshape(-1, 3, 4)
    assert got.shape[0] == moved.shape[0] - 1
    rows = []
    for i in range(1, moved.shape[0]):
        exact = CR.exact_compose(moved[i], moved[0])[1]
        rows.append(CR.within_bounds(got[i - 1], exact, h, w, depths))
    ulps, px, bound = (np.array(c) for c in zip(*rows))
    worst = int(np.argmax(px / bound))
    print("compose %s %s x%g: worst entry %.3g ulp; got %.3g px, ideal %.3g px, ratio to the bound %.3g"
          % (name, m.name, scale, ulps.max(), px[worst], (bound[worst] - 1e-7) / 2.0, (px / bound).max()))
    assert ulps.max() <= 1.0, ulps
    assert (px <= bound).all(), (px, bound)


# ----------------------------------------------------------------------------------------
# b. the fp64 composition
# ----------------------------------------------------------------------------------------
def _compose_f64(ops, proj44):
    """d3d_compose_projections_f64 through the C ABI: float64 [V,4,4] -> float64 [V-1,3,4]."""
    from deep3d_aerial_amd import _lib

    p44 = torch.from_numpy(np.ascontiguousarray(proj44, np.float64)).cuda()
    out = torch.empty((proj44.shape[0] - 1, 12), dtype=torch.float64, device="cuda")
    rc = _lib.load().d3d_compose_projections_f64(ctypes.c_void_p(p44.data_ptr()), int(proj44.shape[0]), ctypes.c_void_p(out.data_ptr()),
                                                 ops._stream())
    _lib.check(rc, "d3d_compose_projections_f64")
    torch.cuda.synchronize()
    return host(out).reshape(-1, 3, 4)


@pytest.mark.parametrize("name", ["small_V5", "aerial"])
@pytest.mark.parametrize("m", MOTIONS, ids=lambda m: m.name)
def test_compose_projections_f64_on_world_cameras(ops, m, name):
    proj, h, w, depths = CR.scene(name)
    moved = CR.move(proj.astype(np.float64), m.G)                      # float64, not rounded to fp32
    assert moved.dtype == np.float64 and not np.array_equal(moved, moved.astype(np.float32))
    got = _compose_f64(ops, moved)
    px, lu = 0.0, 0.0
    for i in range(1, moved.shape[0]):
        exact = CR.exact_compose(moved[i], moved[0])[1]
        px = max(px, CR.displacement_px(got[i - 1], exact, h, w, depths))
        lu = max(lu, CR.displacement_px((moved[i] @ np.linalg.inv(moved[0]))[:3], exact, h, w, depths))
    print("compose f64 %s %s: kernel %.3g px, numpy float64 inv + matmul %.3g px" % (name, m.name, px, lu))
    assert np.isfinite(got).all()
    assert px <= max(16.0 * lu, 1e-12), (px, lu)


# ----------------------------------------------------------------------------------------
# c. the sweeps, end to end
# ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moved_fp32(row, kind, mname):
    """A case of sweep_ref.FP32_ROWS seen from a world frame: the moved fp32 cameras and the float64 volumes of their EXACT
    composition.  Computed once, shared by the families, never written to."""
    sc = R.fp32_scene(row, kind)
    moved = CR.move(sc.proj, CR.motion(mname).G)
    p64 = _exact34(moved)
    return sc, moved, p64, R.variance_volume(sc.feats, p64, sc.depth), R.weighted_corr(sc.feats, p64, sc.weights, sc.depth)


FP32_SWEEPS = [("tiled", R.FP32_ROWS[0], "pixel"), ("direct", R.FP32_ROWS[0], "pixel"), ("direct", R.FP32_ROWS[3], "plane")]


@pytest.mark.parametrize("mname", SWEEP_MOTIONS)
@pytest.mark.parametrize("family,row,kind", FP32_SWEEPS, ids=["%s-%s" % (f, R.fp32_id(r, k)) for f, r, k in FP32_SWEEPS])
def test_fp32_sweeps_from_world_cameras(ops, family, row, kind, mname):
    sc, moved, _, want_var, want_wc = _moved_fp32(row, kind, mname)
    fd, vw, depth = [dev(f) for f in sc.feats], dev(sc.weights), dev(sc.depth)
    p34 = ops.compose_projections(dev(moved))
    var, wc = _run(ops, family, lambda: (ops.variance_volume(fd, p34, depth), ops.weighted_corr(fd, p34, vw, depth)))
    _held("%s %s variance" % (family, mname), host(var), want_var)
    _held("%s %s weighted" % (family, mname), host(wc), want_wc)


@pytest.mark.parametrize("mname", SWEEP_MOTIONS)
def test_window_sweep_from_world_cameras(ops, mname):
    """test_parity_gpu.WINDOW_CASES[2] (ragged patches, two sources on the four-view template, affine hypotheses), built as there."""
    V, C, h, w, D, sweep, yaw, perpix = WINDOW_CASES[2]
    assert perpix
    proj, dv = S.make_scene(V, h, w, max(D, 8), sweep_px=sweep, seed=V + C + D, yaw_deg=yaw)
    feats = S.make_features(V, C, h, w, seed=C + D)
    rng = np.random.default_rng(D + C + h)
    span = float(dv[1] - dv[0])
    cur = (0.5 * (dv[0] + dv[1]) + 0.2 * span * rng.uniform(-1, 1, (h, w))).astype(np.float32)
    depth = ops.depth_range_affine(dev(cur), D, span / 2.0 / D)
    lo, step = host(depth.maps)
    planes = (lo, step, D)
    assert np.array_equal(host(depth.volume()), R.depth_f32(planes, h, w))
    weights = rng.uniform(0.02, 1.0, (V - 1, h, w)).astype(np.float32)
    moved = CR.move(proj, CR.motion(mname).G)
    p64 = _exact34(moved)
    fd, vw = [dev(f) for f in feats], dev(weights)
    p34 = ops.compose_projections(dev(moved))
    var, wc = _run(ops, "window", lambda: (ops.variance_volume(fd, p34, depth), ops.weighted_corr(fd, p34, vw, depth)))
    _held("window %s variance" % mname, host(var), R.variance_volume(feats, p64, planes))
    _held("window %s weighted" % mname, host(wc), R.weighted_corr(feats, p64, weights, planes))


@functools.lru_cache(maxsize=None)
def _moved_fp16(row, mname):
    import oracle

    oracle.build()
    sc = R.fp16_scene(row)
    moved = CR.move(sc.proj, CR.motion(mname).G)
    p64 = _exact34(moved)
    f = sc.feats.astype(np.float32)
    want_oracle = oracle.variance_volume(f[0], f[1:], p64.astype(np.float32), sc.depth_f32())
    return sc, moved, R.variance_volume(sc.feats, p64, sc.depth), want_oracle


@pytest.mark.parametrize("mname", SWEEP_MOTIONS)
@pytest.mark.parametrize("family", ["tiled", "direct"])
def test_fp16_sweep_from_world_cameras(ops, family, mname):
    row = R.FP16_ROWS[2]
    assert R.f16_tiled(row[0], row[1])
    sc, moved, want, want_oracle = _moved_fp16(row, mname)
    fd = [dev(f) for f in sc.feats]
    assert fd[0].dtype == torch.float16
    depth, _ = _depth_dev(ops, sc.depth)
    p34 = ops.compose_projections(dev(moved))
    got = _run(ops, family, lambda: ops.variance_volume(fd, p34, depth))
    _check_fp16("fp16 %s %s variance" % (family, mname), host(got), want, want_oracle)


@pytest.mark.parametrize("mname", SWEEP_MOTIONS)
def test_warps_from_world_cameras(ops, mname):
    """module.homo_warping_float on the moved fp32 pair and ops.homo_warp_double (homo_warping_double, module.py:560-601) on the
    moved float64 pair, against the float64 warp through the exact matrix of the same inputs; test_parity_gpu's warp bound."""
    from deep3d_aerial_amd import module

    sc = R.fp32_scene(R.FP32_ROWS[0], "pixel")
    G = CR.motion(mname).G
    moved, moved64 = CR.move(sc.proj, G), CR.move(sc.proj.astype(np.float64), G)
    depth = dev(sc.depth)
    for i in (1, sc.V - 1):
        src = dev(sc.feats[i])
        got = module.homo_warping_float(src[None], dev(moved[i])[None], dev(moved[0])[None], depth[None])
        assert tuple(got.shape) == (1, sc.C, sc.D, sc.h, sc.w)
        _held("float warp %s view %d" % (mname, i), host(got[0]), R.warp(sc.feats[i], CR.exact_compose(moved[i], moved[0])[0], sc.depth),
              ABS_GATHER, None)
        got = ops.homo_warp_double(src, dev(moved64[i]), dev(moved64[0]), depth)
        _held("double warp %s view %d" % (mname, i), host(got), R.warp(sc.feats[i], CR.exact_compose(moved64[i], moved64[0])[0], sc.depth),
              ABS_GATHER, None)


# ----------------------------------------------------------------------------------------
# d. the models
# ----------------------------------------------------------------------------------------
def _net(tag, g):
    from deep3d_aerial_amd.adamvs import Infer_AdaMVSNet
    from deep3d_aerial_amd.cas_mvsnet import Infer_CascadeMVSNet
    from deep3d_aerial_amd.msrednet import Infer_CascadeREDNet
    from deep3d_aerial_amd.ucsnet import Infer_UCSNet

    ctor = {"casmvsnet": Infer_CascadeMVSNet, "adamvs": Infer_AdaMVSNet, "msrednet": Infer_CascadeREDNet, "ucsnet": Infer_UCSNet}[tag.split("_")[1]]
    return _fill(ctor(num_depth=int(g["num_depth"])), int(g["seed"]))


@pytest.mark.parametrize("tag", CR.MODEL_FIXTURES)
def test_model_forward_on_moved_cameras(ops, tag):
    g = load_golden(tag)
    net = _net(tag, g)
    G = CR.motion(CR.MODEL_MOTION).G
    stages = ("stage1", "stage2", "stage3")
    cams = {"camera frame": {s: dev(g["proj_" + s]) for s in stages}, "moved": {s: dev(CR.move(g["proj_" + s], G)) for s in stages}}
    assert cams["moved"]["stage1"].dtype == torch.float32 and float(cams["moved"]["stage1"].abs().max()) > 1e5
    outs = {}
    with torch.no_grad():
        for k, pm in cams.items():
            outs[k] = net(dev(g["imgs"]), pm, dev(g["depth_values"]))
    keys = [("depth", "_depth"), ("photometric_confidence", "_conf")] + ([("variance", "_variance")] if "ucsnet" in tag else [])
    if "ucsnet" in tag:
        bounds = {"depth": REL_MODEL, "photometric_confidence": 5 * REL_MODEL, "variance": 20 * REL_MODEL}
    else:
        bounds = {"depth": REL_MODEL_FP32, "photometric_confidence": REL_CONF_FP32}
    err = {k: {(s, key): rel_l1(host(out[s][key][0]), g[s + suffix]) for s in stages for key, suffix in keys} for k, out in outs.items()}
    for k, out in outs.items():
        err[k][("final", "depth")] = rel_l1(host(out["depth"][0]), g["depth"])
        if "ucsnet" not in tag:
            err[k][("final", "photometric_confidence")] = rel_l1(host(out["photometric_confidence"][0]), g["photometric_confidence"])
        if "adamvs" in tag:
            vw = torch.stack([t[0, 0] for t in out["stage1"]["pair_confidence"]])
            err[k][("stage1", "view_weights")] = rel_l1(host(vw), g["stage1_view_weights"])
    bounds["view_weights"] = REL_MODEL
    for where in err["moved"]:
        print("%s %s %s: moved %.2e, camera frame %.2e (bound %.0e)" % ((tag,) + where + (err["moved"][where], err["camera frame"][where], bounds[where[1]])))
    assert outs["moved"]["depth"].shape == (1,) + g["depth"].shape
    for where, e in err["moved"].items():
        assert e <= bounds[where[1]], (where, e)
