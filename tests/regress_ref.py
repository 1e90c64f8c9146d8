"""float64 restatements of the operations between the cost volume and the depth map (numpy only).

Written from the reference's formulas -- cas_mvsnet.py:69-76 (soft-argmin, four-plane confidence), ucsnet.py:30-53
(uncertainty_aware_samples) and :137-151 (spread), adamvs.py:478-486 (pair softmax) and :514-525 (online regression),
module.py:616-650 (depth range samples), F.interpolate(bilinear, align_corners=False) -- not from the kernels: every sum is
float64 and nothing here knows how a kernel orders its work.  tests/test_regress_ref.py ties them to the reference's own fp32
outputs (tests/golden) and to ATen on the CPU; tests/test_regress_gpu.py holds the kernels to them.

Two places keep an fp32 step on purpose, because it is part of the operation's definition and not of its error:
  * an affine depth plane is fl(lo + fl(k * step)), the value the [D,h,w] volume would hold (module.py:625-628 in fp32);
  * resize_bilinear computes the source coordinate and the two weights in fp32 as ATen does (a float64 coordinate would differ
    from the reference by the image gradient times one ulp of the coordinate); the blend is float64.
"""
import numpy as np

f32, f64 = np.float32, np.float64

# (h, w, H, W) of every resize the GPU test runs; the CPU test checks the restatement against ATen on the same list
RESIZE_CASES = [(17, 23, 34, 46), (17, 23, 29, 40), (17, 23, 8, 11), (17, 23, 17, 23), (9, 130, 18, 260), (5, 40, 7, 67),
                (1, 1, 5, 6), (6, 9, 1, 1)]


def depth_planes(depth, h, w):
    """[D] | [D,h,w] | (lo [h,w], step [h,w], D) -> float64 [D,h,w]."""
    if isinstance(depth, tuple):
        lo, step, D = depth
        k = np.arange(D, dtype=f32).reshape(-1, 1, 1)
        prod = (k * np.asarray(step, f32)[None]).astype(f32)           # first rounding
        return (np.asarray(lo, f32)[None] + prod).astype(f32).astype(f64)   # second rounding, then widened
    depth = np.asarray(depth, f64)
    if depth.ndim == 1:
        return np.broadcast_to(depth[:, None, None], (depth.shape[0], h, w))
    assert depth.shape[1:] == (h, w)
    return depth


def softmax0(x):
    x = np.asarray(x, f64)
    e = np.exp(x - x.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


class SoftArgmin:
    """depth, conf, index (the float64 expected plane index, before truncation), var (None without lamb), conf_at(k)."""

    def __init__(self, p, dv, lamb):
        D = p.shape[0]
        self.p = p
        self.depth = (p * dv).sum(0)
        self.index = (p * np.arange(D, dtype=f64).reshape(-1, 1, 1)).sum(0)
        self.conf = self.conf_at(np.trunc(self.index).astype(np.int64))       # .long(), then clamp(0, D - 1)
        self.var = None if lamb is None else float(lamb) * np.sqrt((p * (dv - self.depth[None]) ** 2).sum(0))

    def conf_at(self, k):
        """Sum of the probabilities of planes k-1 .. k+2 (the pad=(1, 2) window of four), k an integer or an [h,w] map of
        integers, clamped to 0 .. D-1 as the reference clamps its index; planes outside 0 .. D-1 add nothing."""
        D, h, w = self.p.shape
        k = np.clip(np.broadcast_to(np.asarray(k, np.int64), (h, w)), 0, D - 1)
        out = np.zeros((h, w), f64)
        for j in range(-1, 3):
            kk = k + j
            ok = (kk >= 0) & (kk < D)
            out += np.where(ok, np.take_along_axis(self.p, np.clip(kk, 0, D - 1)[None], 0)[0], 0.0)
        return out


def softargmin(cost, depth, lamb=None):
    cost = np.asarray(cost, f64)
    _, h, w = cost.shape
    return SoftArgmin(softmax0(cost), depth_planes(depth, h, w), lamb)


def pair_softmax_max(score, depth):
    """-> (view_weight = the largest probability, pair_depth = the expected depth)."""
    score = np.asarray(score, f64)
    p = softmax0(score)
    return p.max(0), (p * depth_planes(depth, *score.shape[1:])).sum(0)


def uncertainty_samples(cur, var, D):
    """ucsnet.py:41-51: D hypotheses low + step * i + 1e-12 between cur - var and cur + var."""
    cur, var = np.asarray(cur, f64), np.asarray(var, f64)
    low, high = cur - var, cur + var
    step = (high - low) / (float(D) - 1.0)
    return low[None] + step[None] * np.arange(D, dtype=f64).reshape(-1, 1, 1) + 1e-12


def depth_range_plane(minmax, D):
    """module.py:637-643: D uniform planes from minmax[0] to minmax[-1]."""
    lo, hi = f64(minmax[0]), f64(minmax[-1])
    return lo + np.arange(D, dtype=f64) * ((hi - lo) / (D - 1))


def depth_range_maps(cur, D, interval):
    """module.py:619-623: the (lo, step) maps the D planes of a pixel are generated from."""
    cur = np.asarray(cur, f64)
    lo, hi = cur - D / 2 * f64(interval), cur + D / 2 * f64(interval)
    return lo, (hi - lo) / (D - 1)


def depth_range_pixel(cur, D, interval):
    """module.py:616-630: [h,w] -> [D,h,w]."""
    lo, step = depth_range_maps(cur, D, interval)
    return lo[None] + np.arange(D, dtype=f64).reshape(-1, 1, 1) * step[None]


def _lin_coord(out_size, in_size):
    """Source index pair and weights of one axis, fp32 as ATen's fp32 path computes them (UpSample.h:
    area_pixel_compute_scale / _source_index, guard_index_and_lambda; identical sizes are the identity).

    `scale * (dst + 0.5f) - 0.5f` is ONE rounding: ATen's builds contract it into a fused multiply-add (tests/test_regress_ref.py
    holds this to F.interpolate; with the product rounded on its own, 98 of the 3480 outputs of 17 x 23 -> 29 x 40 came out up to
    8 ulp away, all in the rows and columns where the two coordinates differ by an ulp).  dst + 0.5 is exact, the product of two
    fp32 numbers and the subtraction are exact in float64, so the cast below is that single rounding."""
    dst = np.arange(out_size, dtype=f32)
    scale = f32(in_size) / f32(out_size)
    s = np.maximum(((dst + f32(0.5)).astype(f64) * f64(scale) - 0.5).astype(f32), f32(0))
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = np.clip(s - i0.astype(f32), f32(0), f32(1)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    assert s.dtype == f32 and l1.dtype == f32 and l0.dtype == f32
    return i0, i1, l0.astype(f64), l1.astype(f64)


def resize_bilinear(x, H, W):
    """[n,h,w] or [h,w] -> [n,H,W] / [H,W]: F.interpolate(mode='bilinear', align_corners=False) with size=(H, W)."""
    x = np.asarray(x, f64)
    if x.ndim == 2:
        return resize_bilinear(x[None], H, W)[0]
    _, h, w = x.shape
    y0, y1, hy, ly = _lin_coord(H, h)
    x0, x1, hx, lx = _lin_coord(W, w)
    top = x[:, y0][:, :, x0] * hx + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * hx + x[:, y1][:, :, x1] * lx
    return top * hy[None, :, None] + bot * ly[None, :, None]


def online_start(H, W):
    """(max_p, sum_d, sum_p), all zero (adamvs.py's initial images)."""
    return np.zeros((H, W), f64), np.zeros((H, W), f64), np.zeros((H, W), f64)


def online_update(state, reg, dplane):
    """adamvs.py:514-525 for one plane; a depth plane of another resolution is resampled first (adamvs.py:519-520)."""
    max_p, sum_d, sum_p = state
    reg = np.asarray(reg, f64)
    dplane = np.asarray(dplane, f64)
    if dplane.shape != reg.shape:
        dplane = resize_bilinear(dplane, *reg.shape)
    p = np.exp(reg)
    return np.maximum(max_p, p), dplane * p + sum_d, sum_p + p


def online_finalize(state):
    """adamvs.py:527-529 -> (depth, confidence)."""
    max_p, sum_d, sum_p = state
    e = sum_p + 1e-10
    return sum_d / e, max_p / e
