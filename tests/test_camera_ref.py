"""Ties tests/camera_ref.py down on the CPU, holds the C oracle's composition to it on world-frame cameras, and shows that the
bound the kernel is held to (tests/test_world_cameras_gpu.py) tells a right composition from the reference's fp32 arithmetic.

  exact_compose   src @ inv(ref) @ ref == src in rationals; on the camera-frame scenes it agrees with the oracle and with the
                  reference's own fp32 result (ops_aggregate.npz) within test_compose_projections' bound.
  the C oracle    on every world motion x {make_scene(5, 96, 80, 16, yaw_deg=5), the 688 x 464 frame at f = 1750 px} x stage scale
                  {1, 0.5, 0.25}: every entry within one fp32 ulp of the exact entry, and the displacement over the frame at most
                  twice the ideal rounding's plus 1e-7 px.  The fp32 Gauss-Jordan the oracle used to be missed both on every
                  motion: thousands of ulps on ordinary entries, 1e8 .. 3e9 on an entry that is the remainder of a cancellation,
                  and 1.6 .. 3100 times the displacement bound from 0 km to 100 km.  Even float64 misses the ulp condition (1.7 ulp
                  on the aerial frame under the general rotation: test_float64_arithmetic_misses_the_ulp_condition...), so the
                  oracle composes in binary128; measured now: at most 0.498 ulp and 0.499 of the displacement bound.
  discrimination  numpy's float32 inv + matmul (module.py:528 restated) exceeds the displacement bound on every source view of
                  every motion of 10 km and more: 4.1 .. 180 times at 10 km, 40 .. 1500 times at 100 km (both scenes, all three
                  stage scales).  Below that it is printed, not asserted: 0.26 .. 3.7 times at 0 km, 0.56 .. 15 times at 1 km.
  model fixtures  the precondition of the model tests on moved cameras: moving a fixture's stage matrices by yaw90flip_10km
                  displaces no sample by more than 2.5e-4 px (measured: casmvsnet_v3 7.9e-5, adamvs_v5 1.9e-4, msrednet_v3 1.4e-4,
                  ucsnet_v3 1.6e-4 px, each at stage 3), so no fixture is stepped down from 10 km.
"""
from fractions import Fraction

import numpy as np
import pytest

import camera_ref as CR
import sweep_ref as R
from conftest import load_golden
from deep3d_aerial_amd import synthetic as S

MOTIONS = CR.world_motions()
SCENES = ("small_V5", "aerial")


# ----------------------------------------------------------------------------------------
# the helpers
# ----------------------------------------------------------------------------------------
def test_rne32_and_ulp32():
    one = Fraction(1)
    x = [[one + Fraction(1, 2 ** 24), one + Fraction(3, 2 ** 24), one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80), -one / 3]]
    got = CR.rne32(x)[0]
    assert got[0] == np.float32(1.0) and got[1] == np.float32(1.0 + 2.0 ** -22)        # ties go to the even neighbour
    assert got[2] == np.float32(1.0 + 2.0 ** -23)                                       # past the tie: float64 on the way would lose it
    assert np.float32(float(x[0][2])) == np.float32(1.0)                                # (as here)
    assert got[3] == np.float32(-1.0 / 3.0)
    assert CR.ulp32(one) == Fraction(1, 2 ** 23) and CR.ulp32(one - Fraction(1, 2 ** 60)) == Fraction(1, 2 ** 24)
    assert CR.ulp32(Fraction(-3)) == Fraction(1, 2 ** 22) and CR.ulp32(Fraction(0)) == Fraction(1, 2 ** 149)
    assert CR.ulp32(Fraction(1, 2 ** 140)) == Fraction(1, 2 ** 149)
    for v in (1.0, 1.5, 3.0e8, 7.1e-12):
        assert CR.ulp32(Fraction(v)) == Fraction(float(np.spacing(np.float32(v))))
    err = CR.ulp32_errors(np.full((3, 4), 1.0 + 2.0 ** -23, np.float32), [[one] * 4] * 3)
    assert np.array_equal(err, np.ones((3, 4)))


def test_displacement_px_closed_form_and_direct_projection():
    A = np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
    B = A.copy()
    B[0, 3], B[1, 3] = 3.0, 4.0                      # (u, v) + (3, 4) / d
    assert CR.displacement_px(A, B, 7, 9, [2.0, 4.0]) == pytest.approx(2.5, rel=1e-15)
    assert CR.displacement_px(A, B, 7, 9, [4.0]) == pytest.approx(1.25, rel=1e-15)
    assert CR.displacement_px(A, A, 7, 9, [2.0]) == 0.0
    # a general pair, against the difference of two direct projections (well conditioned in the camera frame)
    proj, h, w, depths = CR.scene("small_V5")
    PA = CR.exact_compose(proj[2], proj[0])[0]
    PB = PA * (1.0 + 1e-6 * np.random.default_rng(0).standard_normal((3, 4)))
    dv = np.broadcast_to(depths[:, None, None], (3, h, w))
    (ua, va), (ub, vb) = R.project(PA, dv), R.project(PB, dv)
    want = float(np.hypot(ua - ub, va - vb).max())
    assert CR.displacement_px(PA, PB, h, w, depths) == pytest.approx(want, rel=1e-6)
    assert CR.displacement_px(CR.exact_compose(proj[2], proj[0])[1], PB, h, w, depths) == pytest.approx(want, rel=1e-6)


def test_world_motions_are_the_ones_the_tests_name():
    assert len(MOTIONS) == 16 and len({m.name for m in MOTIONS}) == 16
    assert sorted({m.offset_m for m in MOTIONS}) == [0.0, 1e3, 1e4, 1e5]
    for m in MOTIONS:
        Rm = m.G[:3, :3]
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-15) and np.linalg.det(Rm) == pytest.approx(1.0)
        assert 100.0 < m.G[2, 3] < 1000.0 and m.G[0, 3] >= m.offset_m
    K_R = np.array([[100.0, 0, 40], [0, 100, 48], [0, 0, 1]]) @ CR.motion("yaw90flip_10km").G[:3, :3].T
    assert K_R[0, 0] == 0.0 and K_R[1, 1] == 0.0                       # the zero diagonal of the 90-degree yaw
    assert CR.motion(CR.MODEL_MOTION).offset_m == 1e4


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_move_keeps_the_relative_geometry(dtype):
    """proj @ inv(G) for every view: the composition of a moved pair is the original one, up to the rounding of the moved matrices
    to their dtype."""
    proj, h, w, depths = CR.scene("small_V5", 0.5)
    proj = proj.astype(dtype)
    assert np.array_equal(CR.move(proj, np.eye(4)), proj)
    for m in MOTIONS:
        moved = CR.move(proj, m.G)
        assert moved.dtype == dtype and moved.shape == proj.shape and np.array_equal(moved[:, 3], proj[:, 3])
        centre = -np.linalg.solve(moved[0, :3, :3].astype(np.float64), moved[0, :3, 3].astype(np.float64))
        assert np.abs(centre - m.G[:3, 3]).max() <= 1e-5 * max(m.offset_m, 1e3)       # the reference camera sits at G's translation
        worst = max(CR.displacement_px(CR.exact_compose(moved[i], moved[0])[1], CR.exact_compose(proj[i], proj[0])[1], h, w, depths)
                    for i in range(1, proj.shape[0]))
        # the moved translation entries are ~ f * offset, rounded to half an ulp; divided by the depth that is the shift in px
        tmax = float(np.abs(moved[:, :3, 3]).max())
        assert worst <= 4.0 * np.finfo(dtype).eps * tmax / depths[0] + (1e-12 if dtype == np.float64 else 1e-7), (m.name, worst)


# ----------------------------------------------------------------------------------------
# exact_compose
# ----------------------------------------------------------------------------------------
def _pairs():
    """(src44, ref44) in both dtypes, camera-frame and moved, scaled rows included."""
    for name, scale in (("small_V5", 1.0), ("aerial", 0.25)):
        proj = CR.scene(name, scale)[0]
        yield proj[1], proj[0]
        for mname in ("flip_1km", "yaw90flip_10km", "general_100km"):
            moved = CR.move(proj, CR.motion(mname).G)
            yield moved[3], moved[0]
            moved64 = CR.move(proj.astype(np.float64), CR.motion(mname).G)
            yield moved64[2], moved64[0]


def test_exact_compose_is_exact():
    n = 0
    for src, ref in _pairs():
        M, exact = CR.exact_compose(src, ref)
        refq = [[Fraction(float(x)) for x in row] for row in ref]
        for r in range(3):
            for c in range(4):
                assert sum(exact[r][k] * refq[k][c] for k in range(4)) == Fraction(float(src[r, c]))      # (src inv(ref)) ref == src
                assert M[r, c] == float(exact[r][c]) and abs(Fraction(float(M[r, c])) - exact[r][c]) <= abs(exact[r][c]) * Fraction(1, 2 ** 53)
        assert M.dtype == np.float64 and M.shape == (3, 4)
        n += 1
    assert n == 14
    with pytest.raises(np.linalg.LinAlgError):
        CR.exact_compose(np.eye(4, dtype=np.float32), np.zeros((4, 4), np.float32))


def test_exact_compose_on_the_camera_frame_scenes(oracle):
    """test_compose_projections' cases and bound (3e-6 of the largest entry): the oracle, and the reference's own fp32 result."""
    for seed in range(4):
        proj, _ = S.make_scene(5, 96, 80, 16, seed=seed, yaw_deg=5.0)
        for i in range(1, 5):
            want = CR.exact_compose(proj[i], proj[0])[0]
            assert np.abs(oracle.compose_proj(proj[i], proj[0]) - want).max() <= 3e-6 * np.abs(want).max()
    g = load_golden("ops_aggregate")
    n = int(g["n_cases"])
    for k in range(n):
        proj, p34 = g["c%d_proj" % k], g["c%d_proj34" % k]
        for i in range(1, proj.shape[0]):
            want = CR.exact_compose(proj[i], proj[0])[0]
            assert np.abs(p34[i - 1] - want).max() <= 3e-6 * np.abs(want).max()
    assert n >= 1


# ----------------------------------------------------------------------------------------
# the C oracle on world-frame cameras
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("m", MOTIONS, ids=lambda m: m.name)
def test_oracle_composes_world_frame_cameras(oracle, m, name):
    worst_ulp, worst_ratio = 0.0, 0.0
    for scale in CR.STAGE_SCALES:
        proj, h, w, depths = CR.scene(name, scale)
        moved = CR.move(proj, m.G)
        for i in range(1, moved.shape[0]):
            exact = CR.exact_compose(moved[i], moved[0])[1]
            ulps, got, bound = CR.within_bounds(oracle.compose_proj(moved[i], moved[0]), exact, h, w, depths)
            worst_ulp, worst_ratio = max(worst_ulp, ulps), max(worst_ratio, got / bound)
            assert ulps <= 1.0, (scale, i, ulps)
            assert got <= bound, (scale, i, got, bound)
    print("oracle %s %s: worst entry %.3g ulp, displacement %.3g of its bound" % (name, m.name, worst_ulp, worst_ratio))


# ----------------------------------------------------------------------------------------
# the bound discriminates
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("m", MOTIONS, ids=lambda m: m.name)
def test_fp32_inverse_and_matmul_miss_the_bound_from_10_km(m, name):
    """module.py:528 restated in numpy float32 -- no kernel computes this.  From 10 km on every source view misses the displacement
    bound the kernel is held to; the ratios below that are printed, not asserted."""
    lo, hi = np.inf, 0.0
    for scale in CR.STAGE_SCALES:
        proj, h, w, depths = CR.scene(name, scale)
        moved = CR.move(proj, m.G)
        for i in range(1, moved.shape[0]):
            exact = CR.exact_compose(moved[i], moved[0])[1]
            _, got, bound = CR.within_bounds(CR.compose_f32_inverse_matmul(moved[i], moved[0]), exact, h, w, depths)
            lo, hi = min(lo, got / bound), max(hi, got / bound)
    print("fp32 inv + matmul %s %s: %.3g .. %.3g times the bound" % (name, m.name, lo, hi))
    if m.offset_m >= 1e4:
        assert lo > 1.0, (m.name, lo, hi)


def _compose_cofactor_float64(src44, ref44):
    """src @ adj(ref) / det(ref) with every operation in IEEE double (Python floats: no fma, no library), one rounding to fp32."""
    m = [[float(x) for x in row] for row in ref44]
    s = [[float(x) for x in row] for row in src44]

    def minor(r, c):
        a = [[m[i][j] for j in range(4) if j != c] for i in range(4) if i != r]
        return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
                + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))

    adj = [[(-1.0) ** (r + c) * minor(c, r) for c in range(4)] for r in range(4)]
    idet = 1.0 / sum(m[0][k] * adj[k][0] for k in range(4))
    return np.array([[sum(s[r][k] * (adj[k][c] * idet) for k in range(4)) for c in range(4)] for r in range(3)]).astype(np.float32)


def test_float64_arithmetic_misses_the_ulp_condition_on_a_cancelled_entry():
    """Why compose_kernel (csrc/compose_dd.h) and the oracle carry more than 53 bits.  Under the general rotation the two source
    views displaced along y have a composed entry [2,0] that is zero for the ideal cameras and 5e-14 .. 1e-13 for their fp32
    roundings: the remainder of terms of 1e-3.  A cofactor inverse in float64 gets it to 1e-16 of the terms -- harmless on the
    image, the displacement stays at the ideal one -- but that is more than an fp32 ulp of the entry."""
    proj, h, w, depths = CR.scene("aerial")
    moved = CR.move(proj, CR.motion("general_10km").G)
    worst = 0.0
    for i in range(1, moved.shape[0]):
        exact = CR.exact_compose(moved[i], moved[0])[1]
        got = _compose_cofactor_float64(moved[i], moved[0])
        ulps = CR.ulp32_errors(got, exact)
        _, px, bound = CR.within_bounds(got, exact, h, w, depths)
        r, c = (int(k) for k in np.unravel_index(np.argmax(ulps), ulps.shape))
        print("view %d: worst entry [%d,%d] %.3g ulp (exact %.3g), displacement %.3g of its bound" % (i, r, c, ulps.max(), float(exact[r][c]), px / bound))
        assert px <= bound
        worst = max(worst, float(ulps.max()))
    assert worst > 1.0


# ----------------------------------------------------------------------------------------
# the model fixtures on moved cameras: the precondition of tests/test_world_cameras_gpu.py
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CR.MODEL_FIXTURES)
def test_model_fixture_precondition(tag):
    """Moving the stage matrices rounds them to fp32 again.  That must leave every sample where it was to well below the kernels'
    coordinate rounding, or the goldens would no longer be the expected output of the moved inputs."""
    g = load_golden(tag)
    H, W = g["imgs"].shape[-2:]
    dv = g["depth_values"][0]
    G = CR.motion(CR.MODEL_MOTION).G
    worst = 0.0
    for stage, scale in CR.MODEL_STAGES:
        proj = g["proj_" + stage][0]
        moved = CR.move(proj, G)
        assert moved.dtype == np.float32 and not np.array_equal(moved, proj)
        assert np.count_nonzero(moved[0, :3, 3]) == 3 and np.abs(moved[0, :3, 3]).max() > 1e5      # no longer K [I|0]
        for i in range(1, proj.shape[0]):
            d = CR.displacement_px(CR.exact_compose(moved[i], moved[0])[1], CR.exact_compose(proj[i], proj[0])[1],
                                   int(H * scale), int(W * scale), CR.frame_depths(dv[0], dv[-1]))
            worst = max(worst, d)
            assert d <= CR.MODEL_PRECONDITION_PX, (stage, i, d)
    print("%s moved by %s: at most %.3g px" % (tag, CR.MODEL_MOTION, worst))
