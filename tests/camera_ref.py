"""The projection composition src_proj @ inverse(ref_proj) (module.py:528-530) in exact rational arithmetic, world-frame cameras
for the tests, and the pixel displacement between two composed matrices.  numpy and fractions only: no torch, no kernel, no oracle
(scene() builds its cameras with deep3d_aerial_amd.synthetic, which is numpy too).

The inputs -- fp32 or fp64 [4,4] matrices -- are exact rationals, so the composition has one exact value.  exact_compose inverts
the reference view's matrix by Gauss-Jordan over fractions.Fraction and multiplies in rationals; nothing rounds until the end.  The
ideal fp32 result is RNE32 of that value (rne32), and an fp32 ulp is taken at it (ulp32).

A rigid motion G of the world (X' = G X) turns every camera P into P @ inv(G): the same relative geometry, seen from a world frame
in which the reference camera sits at G's translation and looks along G's rotation.  The exact composition of the moved pair is the
original one up to the fp32 rounding of the moved matrices; what changes is the arithmetic an implementation has to get through --
sixteen entries of ref_proj that are all in play, and translation entries of 1e5 .. 1e8 that cancel to 1e2 .. 1e5.
"""
import collections
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------
# the exact composition
# ----------------------------------------------------------------------------------------
def _rationals(m44):
    m = np.asarray(m44)
    assert m.shape == (4, 4) and m.dtype in (f32, f64), (m.shape, m.dtype)
    return [[Fraction(float(m[r, c])) for c in range(4)] for r in range(4)]      # (a float is a dyadic rational: no rounding)


def inverse_rational(a):
    """Gauss-Jordan with pivoting (the largest magnitude of the column) on a 4 x 4 of Fractions -> the inverse, in Fractions."""
    n = len(a)
    a = [list(row) + [Fraction(int(r == c)) for c in range(n)] for r, row in enumerate(a)]
    for col in range(n):
        piv = max(range(col, n), key=lambda r: abs(a[r][col]))
        if a[piv][col] == 0:
            raise np.linalg.LinAlgError("singular ref_proj")
        a[col], a[piv] = a[piv], a[col]
        p = a[col][col]
        a[col] = [x / p for x in a[col]]
        for r in range(n):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [x - f * y for x, y in zip(a[r], a[col])]
    return [row[n:] for row in a]


def exact_compose(src44, ref44):
    """(src44 @ inverse(ref44))[:3] -> (float64 [3,4], each entry rounded once; the exact entries, 3 x 4 Fractions)."""
    s, inv = _rationals(src44), inverse_rational(_rationals(ref44))
    exact = [[sum(s[r][k] * inv[k][c] for k in range(4)) for c in range(4)] for r in range(3)]
    return np.array([[float(x) for x in row] for row in exact], f64), exact      # (float(Fraction) rounds correctly)


def rne32(exact):
    """The fp32 value nearest to each exact entry, ties to even -> float32 [3,4] (from the rational, not by way of float64)."""
    out = np.empty((len(exact), len(exact[0])), f32)
    for r, row in enumerate(exact):
        for c, x in enumerate(row):
            g = f32(float(x))
            best = None
            for cand in (np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))):
                if np.isfinite(cand):
                    even = int(np.array(cand, f32).view(np.uint32)) & 1
                    key = (abs(Fraction(float(cand)) - x), even)
                    if best is None or key < best[0]:
                        best = (key, cand)
            out[r, c] = best[1]
    return out


def ulp32(x):
    """The spacing of fp32 at the exact value x (a Fraction): 2^(e - 23) with 2^e <= |x| < 2^(e + 1), never below 2^-149."""
    x = abs(Fraction(x))
    if x == 0:
        return Fraction(1, 2 ** 149)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    return Fraction(2) ** (max(e, -126) - 23)


def ulp32_errors(got, exact):
    """|got - exact| in fp32 ulps of the exact entry -> float64 [3,4]."""
    got = np.asarray(got).reshape(3, 4)
    return np.array([[float(abs(Fraction(float(got[r, c])) - exact[r][c]) / ulp32(exact[r][c])) for c in range(4)] for r in range(3)])


# ----------------------------------------------------------------------------------------
# world-frame cameras
# ----------------------------------------------------------------------------------------
Motion = collections.namedtuple("Motion", "name G offset_m")

FLIP = np.diag([1.0, -1.0, -1.0])                                      # a nadir camera: x east, y south, looking down
YAW90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # exactly 90 degrees: K @ R has a zero diagonal
OFFSETS_M = (0.0, 1e3, 1e4, 1e5)


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _ry(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def _rx(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def rotations():
    return [("identity", np.eye(3)), ("flip", FLIP), ("yaw90flip", YAW90 @ FLIP),
            ("general", _rz(2.5) @ _ry(np.deg2rad(4.0)) @ _rx(np.deg2rad(-3.0)) @ FLIP)]


def world_motions():
    """The rigid motions of the tests: four rotations x four offsets of the camera centres, a few hundred metres up."""
    out = []
    for rname, R in rotations():
        for off in OFFSETS_M:
            G = np.eye(4)
            G[:3, :3] = R
            G[:3, 3] = (off + 123.4, 0.7 * off + 55.5, 550.0)
            out.append(Motion("%s_%gkm" % (rname, off / 1e3), G, off))
    return out


def motion(name):
    return {m.name: m for m in world_motions()}[name]


def move(proj44, G):
    """proj44 [V,4,4] (rows may be scaled: a stage matrix) -> proj44 @ inv(G), in float64, rounded to proj44's dtype."""
    proj44 = np.asarray(proj44)
    assert proj44.shape[-2:] == (4, 4) and proj44.dtype in (f32, f64), (proj44.shape, proj44.dtype)
    G = np.asarray(G, f64)
    R, t = G[:3, :3], G[:3, 3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.array_equal(G[3], [0, 0, 0, 1])
    Ginv = np.eye(4)
    Ginv[:3, :3] = R.T
    Ginv[:3, 3] = -R.T @ t
    return (proj44.astype(f64) @ Ginv).astype(proj44.dtype)


# ----------------------------------------------------------------------------------------
# what a difference between two composed matrices means on the image
# ----------------------------------------------------------------------------------------
def _entries(P):
    """[3,4] array, 12 values, or 3 x 4 Fractions -> 3 x 4 Fractions."""
    if isinstance(P, np.ndarray):
        P = P.reshape(3, 4).tolist()
    return [[x if isinstance(x, Fraction) else Fraction(float(x)) for x in row] for row in P]


def displacement_px(PA, PB, h, w, depths):
    """The largest distance (px) between the source pixel positions the [3,4] matrices PA and PB give, over every reference pixel
    of an h x w frame and the depths.  Either matrix may be given exactly (3 x 4 Fractions).  The difference of the matrices is
    formed in rationals and projected on its own: with A = B + E,  u_A - u_B = (E_x.X - u_B E_z.X) / (A_z.X), which keeps the
    cancellation between rotation and translation (1e8 against 1e8 on a world-frame camera) out of the result."""
    A, B = _entries(PA), _entries(PB)
    E = np.array([[float(a - b) for a, b in zip(ra, rb)] for ra, rb in zip(A, B)], f64)
    A = np.array([[float(x) for x in row] for row in A], f64)
    B = np.array([[float(x) for x in row] for row in B], f64)
    ys, xs = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing="ij")
    d = np.asarray(depths, f64).reshape(-1, 1, 1)

    def apply(M):
        return [(M[r, 0] * xs + M[r, 1] * ys + M[r, 2])[None] * d + M[r, 3] for r in range(3)]

    bx, by, bz = apply(B)
    ex, ey, ez = apply(E)
    az = apply(A)[2]
    du = (ex - bx / bz * ez) / az
    dv = (ey - by / bz * ez) / az
    return float(np.sqrt(du * du + dv * dv).max())


def frame_depths(lo, hi):
    """First, middle and last depth of a sweep."""
    return np.array([lo, 0.5 * (float(lo) + float(hi)), hi], f64)


def within_bounds(got, exact, h, w, depths):
    """The two conditions a composed fp32 matrix is held to, both from the exact entries of the same inputs ->
    (worst entry error in fp32 ulps of the exact entry [bound: 1], displacement of `got` in px, its bound in px): the bound is
    twice the displacement of the ideal result RNE32(exact), plus 1e-7 px."""
    ideal = displacement_px(rne32(exact), exact, h, w, depths)
    return float(ulp32_errors(got, exact).max()), displacement_px(got, exact, h, w, depths), 2.0 * ideal + 1e-7


# ----------------------------------------------------------------------------------------
# the cases the CPU and the GPU tests share
# ----------------------------------------------------------------------------------------
STAGE_SCALES = (1.0, 0.5, 0.25)
MODEL_FIXTURES = ("model_casmvsnet_v3", "model_adamvs_v5", "model_msrednet_v3", "model_ucsnet_v3")
MODEL_MOTION = "yaw90flip_10km"          # every fixture meets MODEL_PRECONDITION_PX at 10 km: none is stepped down
MODEL_PRECONDITION_PX = 2.5e-4           # below the kernels' documented coordinate rounding (3e-4 px)
MODEL_STAGES = (("stage1", 0.25), ("stage2", 0.5), ("stage3", 1.0))


def scene(name, scale=1.0):
    """(proj [V,4,4] fp32 camera-frame, h, w, depths): `small_V<n>` is make_scene(n, 96, 80, 16, yaw_deg=5) at 400 .. 800 m,
    `aerial` a 688 x 464 frame at f = 1750 px and 450 .. 650 m, five views.  `scale` is the stage scale of the first two rows, and
    of the frame."""
    from deep3d_aerial_amd import synthetic as S

    if name == "aerial":
        V, h, w, lo, hi, focal = 5, 464, 688, 450.0, 650.0, 1750.0
    else:
        V, h, w, lo, hi, focal = int(name.split("_V")[1]), 96, 80, 400.0, 800.0, None
    proj, _ = S.make_scene(V, h, w, 16, depth_min=lo, depth_max=hi, focal=focal, yaw_deg=5.0, scale=scale)
    return proj, int(h * scale), int(w * scale), frame_depths(lo, hi)


def compose_f32_inverse_matmul(src44, ref44):
    """The reference's own arithmetic restated in numpy (module.py:528): inverse in fp32, matmul in fp32 -> float32 [3,4]."""
    src44, ref44 = np.asarray(src44, f32), np.asarray(ref44, f32)
    inv = np.linalg.inv(ref44)
    assert inv.dtype == f32
    return np.matmul(src44, inv)[:3].astype(f32)
