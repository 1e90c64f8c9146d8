"""The mesh refinement's rule (deep3d_aerial_amd/refine.py) restated in numpy, its properties, the scene the GPU tests use
(tests/mesh_refine_scene.py) and the plumbing.  tests/test_mesh_refine_gpu.py holds the kernels bit-equal to the functions here."""
import os
import re

import numpy as np
import pytest

import mesh_refine_scene as RS
import test_mesh_clean as MC
import test_mesh_decimate as MD
import test_texture as T
import test_texture_outliers as O

EMPTY = T.EMPTY
RV = 4
QMAX = 3060
DEFAULTS = {"reach": 4, "scales": 2, "scale_step": 0.5, "min_score": 0.6, "min_contrast": 2.0, "smooth": 1.0, "smooth_iterations": 10,
            "depth_tolerance": 0.01}


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def topology_numpy(n, faces):
    """(face_offset, face_index, offset, nbr, fixed): the vertex -> face CSR and the neighbour CSR of the earlier stages."""
    foff, finc = MD.incidence_numpy(n, faces)
    offset, nbr, fixed = MC.adjacency_numpy(n, faces)
    return foff, finc, offset, nbr, fixed


def frames_numpy(vertices, faces, topo):
    """(frame [n, 9] fp64, active [n] uint8)."""
    V = np.asarray(vertices, np.float32).astype(np.float64)
    F = np.asarray(faces, np.int64)
    n = len(V)
    foff, finc, _, _, fixed = topo
    frame, active = np.zeros((n, 9)), np.zeros(n, np.uint8)
    for v in range(n):
        N, used = [0.0, 0.0, 0.0], 0
        for f in finc[foff[v]:foff[v + 1]]:
            ia, ib, ic = F[f]
            if not (0 <= min(ia, ib, ic) and max(ia, ib, ic) < n) or ia == ib or ib == ic or ic == ia:
                continue
            e1, e2 = V[ib] - V[ia], V[ic] - V[ia]
            N[0] += e1[1] * e2[2] - e1[2] * e2[1]
            N[1] += e1[2] * e2[0] - e1[0] * e2[2]
            N[2] += e1[0] * e2[1] - e1[1] * e2[0]
            used += 1
        with np.errstate(all="ignore"):
            L = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
        if not (used > 0 and not fixed[v] and np.isfinite(N).all() and np.isfinite(L) and L > 0):
            continue
        nx, ny, nz = N[0] / L, N[1] / L, N[2] / L
        ax, ay, az = abs(nx), abs(ny), abs(nz)
        j = 0 if ax <= ay and ax <= az else (1 if ay <= az else 2)
        c = [(0.0, -nz, ny), (nz, 0.0, -nx), (-ny, nx, 0.0)][j]
        cl = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        t1 = (c[0] / cl, c[1] / cl, c[2] / cl)
        t2 = (ny * t1[2] - nz * t1[1], nz * t1[0] - nx * t1[2], nx * t1[1] - ny * t1[0])
        frame[v] = (nx, ny, nz) + t1 + t2
        active[v] = 1
    return frame, active


def view_keys_numpy(vertices, frame, active, view, depth_tolerance, reach, step):
    """key [n] int64 of one view: EMPTY where it does not see the vertex."""
    X = np.asarray(vertices, np.float32).astype(np.float64)
    _, _, _, C = T._cam(view)
    H, W = view["depth"].shape
    p2, q2, u, v = T.project(view, X)
    with np.errstate(all="ignore"):
        ok = (active != 0) & (p2 > 0) & (q2 > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        dx, dy, dz = C[0] - X[:, 0], C[1] - X[:, 1], C[2] - X[:, 2]
        dot = (frame[:, 0] * dx + frame[:, 1] * dy) + frame[:, 2] * dz
        ok &= dot > 0
        px = np.clip(np.floor(np.where(ok, u, 0.0) + 0.5), 0, W - 1).astype(np.int64)
        py = np.clip(np.floor(np.where(ok, v, 0.0) + 0.5), 0, H - 1).astype(np.int64)
        D = view["depth"][py, px].astype(np.float32)
        ok &= np.isfinite(D) & (D > 0) & (p2 <= D.astype(np.float64) * (1.0 + depth_tolerance) + float(reach) * step)
        s = 1.0 - dot / np.sqrt((dx * dx + dy * dy) + dz * dz)
        ok &= np.isfinite(s)
    key = T.make_key(np.where(ok, s, 0.0), view["id"])
    return np.where(ok, key, EMPTY)


def views_numpy(vertices, frame, active, views, step, reach=4, depth_tolerance=0.01, lists=None):
    """lists [n, 4] int64: the four smallest distinct keys per vertex, merged into `lists` when given."""
    n = len(vertices)
    cols = [np.full((n, RV), EMPTY, np.int64) if lists is None else np.asarray(lists, np.int64)]
    cols += [view_keys_numpy(vertices, frame, active, v, depth_tolerance, reach, step)[:, None] for v in views]
    allk = np.sort(np.concatenate(cols, 1), 1)
    out = np.full((n, RV), EMPTY, np.int64)
    for i in range(n):
        u = np.unique(allk[i])[:RV]
        out[i, :len(u)] = u
    return out


def greys_numpy(view, P):
    """(q [...] int64, valid [...] bool) of points P [..., 3] fp64 in one view."""
    H, W = view["image"].shape[:2]
    p2, q2, u, v = T.project(view, P)
    with np.errstate(all="ignore"):
        ok = (p2 > 0) & (q2 > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    t = O.tap_numpy(view["image"], np.where(ok, u, 0.0).ravel(), np.where(ok, v, 0.0).ravel())
    q = np.clip(np.floor(4.0 * ((t[:, 0] + t[:, 1]) + t[:, 2]) + 0.5), 0, QMAX).astype(np.int64).reshape(ok.shape)
    return np.where(ok, q, 0), ok


def scores_numpy(vertices, frame, active, lists, views, step, spacing, reach, min_contrast=2.0):
    """(score [n, 2 reach + 1] fp64, used [n, 3] bool, two [n] bool): the scores of the vertices with a used pair (0 elsewhere)."""
    X = np.asarray(vertices, np.float32).astype(np.float64)
    n, nk = len(X), 2 * reach + 1
    Tv = int(np.floor(625.0 * 144.0 * (min_contrast * min_contrast)))
    by_id = {v["id"]: v for v in views if v.get("image") is not None}
    two = (active != 0) & (lists[:, 1] != EMPTY)
    h = (np.arange(nk) - reach).astype(np.float64) * step
    Xk = X[:, None, :] + h[None, :, None] * frame[:, None, 0:3]                         # [n, nk, 3]
    a = (np.arange(25) % 5 - 2).astype(np.float64) * spacing
    b = (np.arange(25) // 5 - 2).astype(np.float64) * spacing
    P = (Xk[:, :, None, :] + a[None, None, :, None] * frame[:, None, None, 3:6]) + b[None, None, :, None] * frame[:, None, None, 6:9]
    q = np.zeros((RV, n, nk, 25), np.int64)
    ok = np.zeros((RV, n, nk), bool)
    for s in range(RV):
        ids = lists[:, s] & 0xffffffff
        for vid, view in by_id.items():
            sel = np.nonzero(two & (lists[:, s] != EMPTY) & (ids == vid))[0]
            if len(sel):
                qs, valid = greys_numpy(view, P[sel])
                q[s, sel], ok[s, sel] = qs, valid.all(-1)
    S, SS = q.sum(-1), (q * q).sum(-1)
    var = 25 * SS - S * S
    z = np.zeros((n, nk, RV - 1))
    pair_ok = np.zeros((n, nk, RV - 1), bool)
    for j in range(1, RV):
        num = 25 * (q[0] * q[j]).sum(-1) - S[0] * S[j]
        good = ok[0] & ok[j] & (var[0] >= Tv) & (var[j] >= Tv)
        with np.errstate(all="ignore"):
            zj = num.astype(np.float64) / np.sqrt(var[0].astype(np.float64) * var[j].astype(np.float64))
        z[:, :, j - 1], pair_ok[:, :, j - 1] = np.where(good, zj, 0.0), good
    used = pair_ok.all(1) & two[:, None]
    score = np.zeros((n, nk))
    for j in range(RV - 1):   # in pair order
        score += np.where(used[:, None, j], z[:, :, j], 0.0)
    cnt = used.sum(1)
    with np.errstate(all="ignore"):
        score = np.where(cnt[:, None] > 0, score / cnt[:, None].astype(np.float64), 0.0)
    return score, used, two


def pairs_lost_numpy(vertices, frame, active, lists, views, step, spacing, reach, min_contrast=2.0):
    """(left [n, 3] bool, dim [n, 3] bool) of the pairs whose two slots hold views: left when at some hypothesis a point of the patch
    is outside one of the pair's images, dim when at some hypothesis where all 50 points are inside va or vb is below Tv."""
    X = np.asarray(vertices, np.float32).astype(np.float64)
    n, nk = len(X), 2 * reach + 1
    Tv = int(np.floor(625.0 * 144.0 * (min_contrast * min_contrast)))
    by_id = {v["id"]: v for v in views}
    h = (np.arange(nk) - reach).astype(np.float64) * step
    a = (np.arange(25) % 5 - 2).astype(np.float64) * spacing
    b = (np.arange(25) // 5 - 2).astype(np.float64) * spacing
    left, dim = np.zeros((n, RV - 1), bool), np.zeros((n, RV - 1), bool)
    for v in np.nonzero((active != 0) & (lists[:, 1] != EMPTY))[0]:
        Xk = X[v][None, :] + h[:, None] * frame[v, None, 0:3]
        P = (Xk[:, None, :] + a[None, :, None] * frame[v, None, None, 3:6]) + b[None, :, None] * frame[v, None, None, 6:9]
        per = [greys_numpy(by_id[int(k & 0xffffffff)], P) if k != EMPTY else None for k in lists[v]]
        var = [None if p is None else 25 * (p[0] * p[0]).sum(-1) - p[0].sum(-1) ** 2 for p in per]
        for j in range(1, RV):
            if per[j] is None:
                continue
            inside = per[0][1].all(-1) & per[j][1].all(-1)
            left[v, j - 1] = not inside.all()
            dim[v, j - 1] = (inside & ((var[0] < Tv) | (var[j] < Tv))).any()
    return left, dim


def match_numpy(vertices, frame, active, lists, views, step, spacing=None, reach=4, min_score=0.6, min_contrast=2.0):
    """(kstar [n] int32, weight [n] fp32, d0 [n] fp32, counts [4] int32)."""
    spacing = step if spacing is None else spacing
    score, used, two = scores_numpy(vertices, frame, active, lists, views, step, spacing, reach, min_contrast)
    n = len(score)
    kstar, weight, d0 = np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for v in np.nonzero(used.any(1))[0]:
        s = score[v]
        k = min(range(2 * reach + 1), key=lambda k: (-s[k], abs(k - reach), k))
        delta = 0.0
        if 0 < k < 2 * reach:
            den = (s[k - 1] - 2.0 * s[k]) + s[k + 1]
            if den < 0:
                delta = min(max(0.5 * (s[k - 1] - s[k + 1]) / den, -0.5), 0.5)
        kstar[v] = k
        weight[v] = 0.0 if s[k] < min_score else 1.0
        d0[v] = np.float32((float(k - reach) + delta) * step)
    counts = np.array([(active != 0).sum(), two.sum(), used.any(1).sum(), (weight != 0).sum()], np.int32)
    return kstar, weight, d0, counts


def relax_numpy(weight, d0, active, topo, smooth=1.0, iterations=10):
    """d [n] fp32 after the Jacobi steps, every operation in fp32."""
    _, _, offset, nbr, _ = topo
    n = len(weight)
    act = active != 0
    lam = np.float32(smooth)
    w, d0 = weight.astype(np.float32), d0.astype(np.float32)
    deg = np.diff(offset)
    d = np.where(act, w * d0, np.float32(0.0)).astype(np.float32)
    for _ in range(iterations):
        total = np.zeros(n, np.float32)
        for j in range(int(deg.max()) if n else 0):   # the j-th neighbour of every vertex that has one: CSR order per vertex
            has = deg > j
            total[has] = total[has] + d[nbr[offset[:-1][has] + j]]
        with np.errstate(all="ignore"):
            mean = np.where(deg > 0, total / deg.astype(np.float32), np.float32(0.0)).astype(np.float32)
            new = ((w * d0 + lam * mean) / (w + lam)).astype(np.float32)
        d = np.where(act, new, np.float32(0.0)).astype(np.float32)
    return d


def apply_numpy(vertices, frame, active, d):
    V = np.asarray(vertices, np.float32)
    moved = (V.astype(np.float64) + d.astype(np.float64)[:, None] * frame[:, 0:3]).astype(np.float32)
    return np.where((active != 0)[:, None], moved, V)


def refine_numpy(vertices, faces, views, step, spacing=None, reach=4, scales=2, scale_step=0.5, min_score=0.6, min_contrast=2.0, smooth=1.0,
                 smooth_iterations=10, depth_tolerance=0.01, detail=None):
    """The refined vertices [n, 3] fp32; detail (a list) gets every scale's intermediate arrays."""
    V = np.asarray(vertices, np.float32)
    topo = topology_numpy(len(V), faces)
    spacing = step if spacing is None else spacing
    for _ in range(scales):
        frame, active = frames_numpy(V, faces, topo)
        lists = views_numpy(V, frame, active, views, step, reach, depth_tolerance)
        kstar, weight, d0, counts = match_numpy(V, frame, active, lists, views, step, spacing, reach, min_score, min_contrast)
        d = relax_numpy(weight, d0, active, topo, smooth, smooth_iterations)
        out = apply_numpy(V, frame, active, d)
        if detail is not None:
            detail.append({"vertices": V, "frame": frame, "active": active, "lists": lists, "kstar": kstar, "weight": weight, "d0": d0,
                           "counts": counts, "d": d, "out": out, "step": step, "spacing": spacing})
        V = out
        step, spacing = step * scale_step, spacing * scale_step
    return V


# ----------------------------------------------------------------------------------------
# the scene (shared with the GPU tests: computed once)
# ----------------------------------------------------------------------------------------
_SCENE = {}


def scene():
    """The scene's mesh and views, and the restatement's chain on it with the scene's settings and every default."""
    if not _SCENE:
        V0, F, true, interior = RS.displaced_mesh()
        vs = RS.numpy_views()
        detail = []
        out = refine_numpy(V0, F, vs, RS.STEP, RS.SPACING, detail=detail)
        _SCENE.update(V0=V0, F=F, true=true, interior=interior, views=vs, detail=detail, out=out)
    return _SCENE


def rms_ratio(V0, out, active):
    before = np.sqrt((RS.plane_distance(V0)[active] ** 2).mean())
    after = np.sqrt((RS.plane_distance(out)[active] ** 2).mean())
    return before, after


def test_the_scene_holds_every_crafted_case():
    s = scene()
    V0, F, vs, d = s["V0"], s["F"], s["views"], s["detail"][0]
    n = len(V0)
    assert n == RS.NX * RS.NY + 2 and n % 16 != 0 and (RS.NX * RS.NY) % 16 != 0 and len(vs) == 7 and vs[0]["image"].shape == (96, 128, 3)
    active, lists, kstar, weight = d["active"] != 0, d["lists"], d["kstar"], d["weight"]
    topo = topology_numpy(n, F)
    fixed = topo[4] != 0
    _, _, idx, (lone, free) = RS.grid_mesh()
    # boundary vertices, a vertex with only a degenerate face, an unreferenced vertex: inactive
    border = np.setdiff1d(idx.ravel(), idx[1:-1, 1:-1].ravel())
    assert fixed[border].all() and not active[border].any()
    assert not active[lone] and (F == lone).any(1).sum() == 1 and not active[free] and not (F == free).any()
    assert np.array_equal(active[:RS.NX * RS.NY], s["interior"][:RS.NX * RS.NY])
    # the displacement is within 0.75 reach step
    off = RS.plane_distance(V0)
    assert off[active].max() <= 0.75 * RS.REACH * RS.STEP + 1e-3 and off[active].max() > 0.7 * RS.REACH * RS.STEP and (off[~active] < 1e-3).all()
    # a vertex seen by fewer than two views
    few = active & (lists[:, 1] == EMPTY)
    assert few.any() and (kstar[few] == -1).all()
    # a vertex whose patch leaves an image at some hypothesis, so a pair is dropped while another is used
    score, used, two = scores_numpy(V0, d["frame"], d["active"], lists, vs, RS.STEP, RS.SPACING, RS.REACH)
    left, dim = pairs_lost_numpy(V0, d["frame"], d["active"], lists, vs, RS.STEP, RS.SPACING, RS.REACH)
    assert not (used & (left | dim)).any()
    dropped = two & used.any(1) & (left & ~dim).any(1)   # a pair lost to the image border alone, with contrast to spare, beside a used one
    assert dropped.any()
    # a patch on the region painted uniform: two views or more, no used pair
    flat = two & ~used.any(1) & ((V0[:, 0] - RS.UNIFORM[0]) ** 2 + (V0[:, 1] - RS.UNIFORM[1]) ** 2 < (RS.UNIFORM[2] - 12.0) ** 2)
    assert flat.any() and (kstar[flat] == -1).all()
    # a vertex whose best hypothesis is an end of the range
    ends = (kstar == 0) | (kstar == 2 * RS.REACH)
    assert ends.any()
    print("scene: %d vertices, %d active, %d with two views, %d matched, %d moved; %d with a dropped pair, %d at an end, %d below min_score"
          % (n, d["counts"][0], d["counts"][1], d["counts"][2], d["counts"][3], dropped.sum(), ends.sum(), ((kstar >= 0) & (weight == 0)).sum()))
    assert d["counts"][0] == active.sum() and d["counts"][3] > 0.8 * active.sum()


def test_refinement_halves_the_distance_to_the_true_surface():
    """The effect on the scene with its settings and every default: the RMS distance of the active interior vertices to the true
    plane after the restatement's two scales is at most half of what it was."""
    s = scene()
    active = s["detail"][0]["active"] != 0
    assert np.array_equal(active, s["interior"])
    before, after = rms_ratio(s["V0"], s["out"], active)
    mid = rms_ratio(s["V0"], s["detail"][0]["out"], active)[1]
    print("rms distance to the plane: %.4f before, %.4f after one scale, %.4f after two (ratio %.4f)" % (before, mid, after, after / before))
    assert after <= 0.5 * before
    # nothing but positions of active vertices changed
    assert np.array_equal(s["out"][~active].view(np.uint32), s["V0"][~active].view(np.uint32))


def test_the_view_lists_do_not_depend_on_view_order_or_batching():
    s = scene()
    d = s["detail"][0]
    vs = s["views"]
    want = d["lists"]
    assert (np.diff(want, axis=1)[want[:, 1:] != EMPTY] > 0).all()
    assert np.array_equal(views_numpy(s["V0"], d["frame"], d["active"], vs[::-1], RS.STEP), want)
    half = views_numpy(s["V0"], d["frame"], d["active"], vs[4:], RS.STEP)
    assert not np.array_equal(half, want)
    assert np.array_equal(views_numpy(s["V0"], d["frame"], d["active"], vs[:4], RS.STEP, lists=half), want)
    # a key's high word is 1 - cos of a front-facing view: in 0 .. 1
    s0 = (want[want != EMPTY] >> 32).astype(np.uint32).view(np.float32)
    assert (s0 >= 0).all() and (s0 < 1).all()


def test_frames_are_orthonormal_and_follow_the_smallest_axis():
    s = scene()
    fr, active = s["detail"][0]["frame"], s["detail"][0]["active"] != 0
    n, t1, t2 = fr[active, 0:3], fr[active, 3:6], fr[active, 6:9]
    for a, b in ((n, n), (t1, t1), (t2, t2)):
        assert np.abs((a * b).sum(1) - 1).max() < 1e-14
    for a, b in ((n, t1), (n, t2), (t1, t2)):
        assert np.abs((a * b).sum(1)).max() < 1e-14
    assert (n @ RS.PLANE_N > 0).all()   # towards the cameras, however rough the displaced mesh is
    assert not fr[~active].any()
    # ties go to the lowest axis; a zero component of e_j x n is +0
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [-1, 0, 0], [0, -1, 0], [-1, -1, 0], [1, -1, 0], [-1, 1, 0]], np.float32)
    F = np.array([[0, 1, 3], [0, 3, 2], [0, 2, 8], [0, 8, 4], [0, 4, 6], [0, 6, 5], [0, 5, 7], [0, 7, 1]], np.int32)
    fr, act = frames_numpy(V, F, topology_numpy(9, F))
    assert act.tolist() == [1] + [0] * 8
    assert fr[0].tolist() == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0] and not np.signbit(fr[0][3])


def test_the_pick_prefers_the_centre_on_ties_and_fits_a_parabola():
    V = np.zeros((1, 3), np.float32)
    frame = np.array([[0, 0, 1, 0, -1, 0, 1, 0, 0]], np.float64)

    def pick(scores, reach=2, min_score=0.6, step=0.5):
        import unittest.mock as mock

        with mock.patch(__name__ + ".scores_numpy", lambda *a, **k: (np.array([scores], np.float64), np.array([[True, False, False]]),
                                                                     np.array([True]))):
            k, w, d0, counts = match_numpy(V, frame, np.ones(1, np.uint8), np.zeros((1, RV), np.int64), [], step, reach=reach,
                                           min_score=min_score)
        return int(k[0]), float(w[0]), float(d0[0])

    assert pick([0.7, 0.9, 0.9, 0.9, 0.7]) == (2, 1.0, 0.0)              # a flat top: the centre, den = 0, no delta
    assert pick([0.9, 0.7, 0.7, 0.7, 0.9]) == (0, 1.0, -1.0)             # equal |k - reach|: the smaller k, an end: no delta
    assert pick([0.1, 0.8, 0.9, 0.8, 0.1]) == (2, 1.0, 0.0)              # symmetric: delta 0
    k, w, d0 = pick([0.1, 0.6, 0.9, 0.8, 0.1])
    assert (k, w) == (2, 1.0) and d0 == np.float32(0.5 * (0.5 * (0.6 - 0.8) / ((0.6 - 1.8) + 0.8)))
    assert pick([0.1, 0.2, 0.5, 0.2, 0.1]) == (2, 0.0, 0.0)              # below min_score: weight 0
    assert pick([0.1, 0.2, 0.3, 0.9, 0.9])[0] == 3                       # nearer the centre
    assert pick([0.0, 0.9, 0.9, 0.0, 0.0], step=1.0) == (2, 1.0, -0.5)            # a tie with a neighbour: half a step towards it, the bound


def test_relaxation_fills_in_unmatched_vertices_and_holds_inactive_ones():
    # a path 0 - 1 - 2 - 3 - 4 as a fan of faces is awkward: use the CSR directly
    offset = np.array([0, 1, 3, 5, 7, 8], np.int64)
    nbr = np.array([1, 0, 2, 1, 3, 2, 4, 3], np.int32)
    topo = (None, None, offset, nbr, None)
    w = np.array([0, 1, 0, 1, 0], np.float32)
    d0 = np.array([9, 1, 9, 1, 9], np.float32)
    active = np.array([0, 1, 1, 1, 0], np.uint8)
    assert relax_numpy(w, d0, active, topo, 1.0, 0).tolist() == [0, 1, 0, 1, 0]
    one = relax_numpy(w, d0, active, topo, 1.0, 1)
    assert one.tolist() == [0.0, 0.5, 1.0, 0.5, 0.0]   # the unmatched vertex takes its neighbours' mean, the ends stay 0
    many = relax_numpy(w, d0, active, topo, 1.0, 200)
    assert many[0] == 0 and many[4] == 0 and 0 < many[2] < 1 and abs(many[1] - (1 + many[2] / 2) / 2) < 1e-6
    assert relax_numpy(w, d0, active, topo, 1e-6, 50)[1] == pytest.approx(1.0, abs=1e-5)   # a vanishing weight keeps the data


# ----------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------
NAMES = ["d3d_mesh_refine_views_max", "d3d_mesh_refine_frames", "d3d_mesh_refine_views", "d3d_mesh_refine_match", "d3d_mesh_refine_relax",
         "d3d_mesh_refine_apply"]


def test_the_header_carries_the_entry_points_and_abi_11():
    from deep3d_aerial_amd import _lib, refine

    text = open(_lib.HEADER).read()
    assert re.search(r"#define D3D_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, text) and n in _lib.SIGNATURES, n
    assert "mesh_refine.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "does not claim to match" in refine.__doc__ and "settings, not measurements" in refine.__doc__


def test_the_library_refuses_bad_arguments_and_no_vertices():
    import ctypes

    from deep3d_aerial_amd import _lib

    lib = _lib.load()
    assert lib.d3d_mesh_refine_views_max() == RV
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before a launch
    g = lambda kw, k, d: kw[k] if k in kw else d
    frames = lambda **kw: lib.d3d_mesh_refine_frames(g(kw, "v", p), g(kw, "n", 4), g(kw, "f", p), g(kw, "m", 4), g(kw, "foff", p),
                                                     g(kw, "finc", p), g(kw, "fixed", p), g(kw, "frame", p), g(kw, "active", p), None)
    for bad in ({"v": None}, {"f": None}, {"foff": None}, {"finc": None}, {"fixed": None}, {"frame": None}, {"active": None}, {"n": 0},
                {"n": -1}, {"n": 1 << 31}, {"m": -1}, {"m": 1 << 29}):
        assert frames(**bad) == -1, bad
    views = lambda **kw: lib.d3d_mesh_refine_views(g(kw, "v", p), g(kw, "n", 4), g(kw, "frame", p), g(kw, "active", p), g(kw, "views", p),
                                                   g(kw, "nv", 3), g(kw, "tol", 0.01), g(kw, "reach", 4), g(kw, "step", 0.5), g(kw, "list", p),
                                                   None)
    for bad in ({"v": None}, {"frame": None}, {"active": None}, {"views": None}, {"list": None}, {"n": 0}, {"n": -1}, {"nv": -1},
                {"nv": 1 << 20}, {"tol": -0.1}, {"tol": float("nan")}, {"reach": 0}, {"reach": 8}, {"step": 0.0}, {"step": float("inf")}):
        assert views(**bad) == -1, bad
    match = lambda **kw: lib.d3d_mesh_refine_match(g(kw, "v", p), g(kw, "n", 4), g(kw, "frame", p), g(kw, "active", p), g(kw, "list", p),
                                                   g(kw, "views", p), g(kw, "nv", 3), g(kw, "reach", 4), g(kw, "step", 0.5),
                                                   g(kw, "spacing", 0.5), g(kw, "tv", 360000), g(kw, "min_score", 0.6), g(kw, "kstar", p),
                                                   g(kw, "weight", p), g(kw, "d0", p), g(kw, "counts", p), None)
    for bad in ({"v": None}, {"frame": None}, {"active": None}, {"list": None}, {"views": None}, {"kstar": None}, {"weight": None},
                {"d0": None}, {"counts": None}, {"n": 0}, {"n": 1 << 27}, {"nv": -1}, {"reach": 0}, {"reach": 8}, {"step": -1.0},
                {"step": float("nan")}, {"spacing": 0.0}, {"tv": 0}, {"min_score": 1.5}, {"min_score": float("nan")}):
        assert match(**bad) == -1, bad
    assert match(reach=8) == -1 and b"reach=8" in lib.d3d_last_error()
    relax = lambda **kw: lib.d3d_mesh_refine_relax(g(kw, "w", p), g(kw, "d0", ctypes.c_void_p(512)), g(kw, "active", p), g(kw, "offset", p),
                                                   g(kw, "nbr", p), g(kw, "n", 4), g(kw, "lam", 1.0), g(kw, "its", 10),
                                                   g(kw, "work", ctypes.c_void_p(768)), g(kw, "out", ctypes.c_void_p(1024)), None)
    for bad in ({"w": None}, {"d0": None}, {"active": None}, {"offset": None}, {"nbr": None}, {"work": None}, {"out": None}, {"n": 0},
                {"lam": 0.0}, {"lam": float("nan")}, {"its": -1}, {"work": ctypes.c_void_p(1024)}, {"out": ctypes.c_void_p(512)}):
        assert relax(**bad) == -1, bad
    apply = lambda **kw: lib.d3d_mesh_refine_apply(g(kw, "v", p), g(kw, "n", 4), g(kw, "frame", p), g(kw, "active", p), g(kw, "d", p),
                                                   g(kw, "out", p), None)
    for bad in ({"v": None}, {"frame": None}, {"active": None}, {"d": None}, {"out": None}, {"n": 0}, {"n": -1}):
        assert apply(**bad) == -1, bad


def test_settings_are_checked():
    from deep3d_aerial_amd import refine

    s = refine.check_refine_settings({"step": 0.5})
    assert s == dict(DEFAULTS, step=0.5, spacing=0.5, views_per_batch=None)
    assert refine.check_refine_settings({"step": 2, "spacing": 3, "reach": 7, "scales": 8})["spacing"] == 3.0
    assert refine.min_variance(2.0) == 360000
    for bad in ({}, {"step": 0}, {"step": -1}, {"step": float("nan")}, {"step": float("inf")}, {"step": 1, "reach": 0}, {"step": 1, "reach": 8},
                {"step": 1, "reach": 2.5}, {"step": 1, "scales": 0}, {"step": 1, "scales": 9}, {"step": 1, "spacing": 0},
                {"step": 1, "spacing": float("nan")}, {"step": 1, "scale_step": 0}, {"step": 1, "scale_step": 1.5},
                {"step": 1, "scale_step": float("nan")}, {"step": 1, "min_score": 2}, {"step": 1, "min_score": float("nan")},
                {"step": 1, "min_contrast": 0}, {"step": 1, "min_contrast": 1e-4}, {"step": 1, "min_contrast": float("inf")},
                {"step": 1, "smooth": 0}, {"step": 1, "smooth": float("nan")}, {"step": 1, "smooth_iterations": -1},
                {"step": 1, "depth_tolerance": -1}, {"step": 1, "depth_tolerance": float("nan")}, {"step": 1, "views_per_batch": 0},
                {"step": 1, "reech": 4}):
        with pytest.raises(ValueError):
            refine.check_refine_settings(bad)
    import torch

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.refine_mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), [], 0.5)
    with pytest.raises(ValueError):
        refine.refine_mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), [], 0.0)


def test_the_flags_parse_and_asking_without_a_mesh_is_an_argument_error():
    from deep3d_aerial_amd import predict, refine

    base = ["--mesh", "m.ply", "--mvs", "x", "--out", "o.ply"]
    for bad in ([], ["--step", "0"], ["--step", "nan"], ["--step", "1", "--reach", "8"], ["--step", "1", "--scales", "0"],
                ["--step", "1", "--min_contrast", "0"]):
        with pytest.raises(SystemExit):
            refine.main(base + bad)
    pbase = ["--output_folder", "out", "--synthetic_items", "2", "--random_weights", "--fuse"]
    mesh = ["--mesh", "m.ply", "--mesh_border=0,1,0,1,0,1", "--mesh_voxel=0.5"]
    assert predict._mesh_settings(predict.parse_args(pbase + mesh)).get("refine") is None
    a = predict.parse_args(pbase + mesh + ["--mesh_refine", "0.25", "--mesh_refine_reach", "3", "--mesh_refine_scales", "1",
                                           "--mesh_refine_smooth_iterations", "4"])
    r = predict._mesh_settings(a)["refine"]
    assert r["step"] == 0.25 and r["reach"] == 3 and r["scales"] == 1 and r["smooth_iterations"] == 4 and r["spacing"] is None
    assert refine.check_refine_settings(r)["spacing"] == 0.25
    with pytest.raises(SystemExit):
        predict.parse_args(pbase + ["--mesh_refine", "0.25"])   # without --mesh
    for bad in (["--mesh_refine", "0"], ["--mesh_refine", "0.25", "--mesh_refine_reach", "0"], ["--mesh_refine", "0.25", "--mesh_refine_scales", "9"]):
        with pytest.raises(SystemExit):
            predict.parse_args(pbase + mesh + bad)
