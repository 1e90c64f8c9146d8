"""Helper of the view-selection tests (not a test module): a restatement of the rule of deep3d_aerial_amd/view_selection.py in
plain Python and numpy, hand-made and synthetic sparse models, and the canonical form in which its files are compared with the
reference's.  The restatement shares one thing with the module under test: view_selection.angle_table, the single copy of the
table (the rule is "search the table you are handed")."""
import math
import os

import numpy as np

from deep3d_aerial_amd import sparse_model, view_selection

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_selection")
SCENES = ("sparse", "dense")
BLOCK_SIZE, OVERLAP = (200.0, 200.0, 50.0), 4    # what the goldens were made with


# ----------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------
def make_model(images, points, centers=None):
    """A SparseModel from {image id: [point ids]} (-1: no point) and {point id: ((x, y, z), [image ids])}; centers
    {image id: (x, y, z)} (default: the origin), stored as an identity rotation and t = -C."""
    ids = sorted(images)
    pids = sorted(points)
    off = np.concatenate([[0], np.cumsum([len(images[i]) for i in ids])]).astype(np.int64)
    obs = np.array([p for i in ids for p in images[i]], np.int64).reshape(-1)
    toff = np.concatenate([[0], np.cumsum([len(points[p][1]) for p in pids])]).astype(np.int64)
    trk = np.array([k for p in pids for k in points[p][1]], np.int64).reshape(-1)
    xyz = np.array([points[p][0] for p in pids], np.float64).reshape(-1, 3)
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (len(ids), 1))
    t = -np.array([(centers or {}).get(i, (0.0, 0.0, 0.0)) for i in ids], np.float64).reshape(-1, 3)
    return sparse_model.SparseModel(np.array(ids, np.int64), q, t, ["%d.jpg" % i for i in ids], off, obs, np.array(pids, np.int64), xyz,
                                    toff, trk)


def consistent(images_of_point, xyz=None, centers=None):
    """make_model from {point id: [image ids]} alone: every image observes each point once per entry of its track."""
    images = {}
    for p in sorted(images_of_point):
        for k in images_of_point[p]:
            images.setdefault(k, []).append(p)
    points = {p: ((xyz or {}).get(p, (float(p), 0.0, 0.0)), list(ks)) for p, ks in images_of_point.items()}
    return make_model(images, points, centers)


def shuffled(model, seed):
    """The same model with the observations within every image and the entries within every track in another order."""
    rng = np.random.default_rng(seed)
    obs, trk = model.obs_point.copy(), model.trk_image.copy()
    for off, arr in ((model.img_offset, obs), (model.trk_offset, trk)):
        for a, b in zip(off[:-1], off[1:]):
            arr[a:b] = rng.permutation(arr[a:b])
    return sparse_model.SparseModel(model.image_ids, model.qvec, model.tvec, model.names, model.img_offset, obs, model.point_ids, model.xyz,
                                    model.trk_offset, trk)


def write_text(model, folder, image_order=None, point_order=None):
    """The model as images.txt and points3D.txt, the images and points in the given orders of dense indices."""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "images.txt"), "w") as f:
        f.write("# images\n")
        for k in (range(model.n_img) if image_order is None else image_order):
            f.write("%d %s %s 1 %s\n" % (model.image_ids[k], " ".join(repr(float(v)) for v in model.qvec[k]),
                                         " ".join(repr(float(v)) for v in model.tvec[k]), model.names[k]))
            f.write(" ".join("0.5 0.5 %d" % p for p in model.obs_point[model.img_offset[k]:model.img_offset[k + 1]]) + "\n")
    with open(os.path.join(folder, "points3D.txt"), "w") as f:
        f.write("# points\n")
        for p in (range(model.n_pts) if point_order is None else point_order):
            track = model.trk_image[model.trk_offset[p]:model.trk_offset[p + 1]]
            f.write("%d %s 0 0 0 0.5 %s\n" % (model.point_ids[p], " ".join(repr(float(v)) for v in model.xyz[p]),
                                              " ".join("%d 0" % k for k in track)))


def strip_flight(n_strips, per_strip, points_per_image, seed=0):
    """A synthetic nadir block as dense arrays (tools/view_selection_bench.py and the tests): cameras on n_strips lines, a ground
    point seen by the cameras whose footprint holds it."""
    rng = np.random.default_rng(seed)
    sx, sy, half_x, half_y, height = 50.0, 90.0, 75.0, 100.0, 300.0
    cx, cy = np.meshgrid(np.arange(per_strip) * sx, np.arange(n_strips) * sy)
    centers = np.stack([cx.ravel(), cy.ravel(), np.full(cx.size, height)], 1)
    n_img = centers.shape[0]
    density = points_per_image / (4 * half_x * half_y)
    w, h = (per_strip - 1) * sx + 2 * half_x, (n_strips - 1) * sy + 2 * half_y
    n_pts = int(density * w * h)
    xyz = np.stack([rng.uniform(-half_x, w - half_x, n_pts), rng.uniform(-half_y, h - half_y, n_pts), rng.normal(0, 5, n_pts)], 1)
    i0 = np.clip(np.ceil((xyz[:, 0] - half_x) / sx), 0, per_strip).astype(np.int64)
    i1 = np.clip(np.floor((xyz[:, 0] + half_x) / sx) + 1, 0, per_strip).astype(np.int64)
    j0 = np.clip(np.ceil((xyz[:, 1] - half_y) / sy), 0, n_strips).astype(np.int64)
    j1 = np.clip(np.floor((xyz[:, 1] + half_y) / sy) + 1, 0, n_strips).astype(np.int64)
    nx, ny = np.maximum(i1 - i0, 0), np.maximum(j1 - j0, 0)
    length = nx * ny
    toff = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    owner = np.repeat(np.arange(n_pts), length)
    e = np.arange(toff[-1]) - toff[owner]
    trk = ((j0[owner] + e // np.maximum(nx[owner], 1)) * per_strip + i0[owner] + e % np.maximum(nx[owner], 1)).astype(np.int64)
    order = np.argsort(trk, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(trk, minlength=n_img))]).astype(np.int64)
    ids, pids = np.arange(1, n_img + 1, dtype=np.int64), np.arange(1, n_pts + 1, dtype=np.int64)
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n_img, 1))
    return sparse_model.SparseModel(ids, q, -centers, ["%d.jpg" % i for i in ids], off, pids[owner[order]], pids, xyz, toff, ids[trk])


# ----------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------
def blocks(model, base_size=None, overlap=1, border=None):
    x, y, z = (np.percentile(model.xyz[:, a], [0.5, 99.5]) for a in range(3))
    scene = list(border) if border is not None else [x[0], x[1], y[0], y[1], z[0], z[1]]
    size = [float(v) for v in base_size] if base_size is not None else [(x[1] - x[0]) / 2.0, (y[1] - y[0]) / 2.0, (z[1] - z[0]) / 1.0]
    out = []
    for j in range(math.ceil((scene[3] - scene[2]) / size[1])):
        for i in range(math.ceil((scene[1] - scene[0]) / size[0])):
            x0 = scene[0] + i * size[0] - overlap
            y0 = scene[2] + j * size[1] - overlap
            out.append([x0, x0 + size[0] + overlap, y0, y0 + size[1] + overlap, z[0], z[1]])
    return out, scene


def references(model, block_list):
    """bool [n_blocks, n_img]."""
    index = {int(i): k for k, i in enumerate(model.image_ids)}
    mask = np.zeros((len(block_list), model.n_img), bool)
    for b, r in enumerate(block_list):
        for p in range(model.n_pts):
            if model.point_ids[p] > 0 and r[0] < model.xyz[p, 0] < r[1] and r[2] < model.xyz[p, 1] < r[3]:
                for k in model.trk_image[model.trk_offset[p]:model.trk_offset[p + 1]]:
                    mask[b, index[int(k)]] = True
    return mask


def weight(c_r, c_s, x, edge, w):
    a, b = c_r - x, c_s - x
    la = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    lb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    if la == 0.0 or lb == 0.0:
        return 0
    c = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (np.sqrt(la) * np.sqrt(lb))
    k = 0
    for j in range(len(edge)):   # the largest k with c <= edge[k]; 0 when there is none
        if c <= edge[j]:
            k = j
    return int(w[k])


def _bin_fast(c, edge):
    return max(int(np.searchsorted(-edge, -c, side="right")) - 1, 0)   # the same k for a table that does not increase


def rows(model, r, mode="points", angle=view_selection.ANGLE_DEFAULT):
    """(C, S) of the image id r as {image id: sum}; S is C in points mode."""
    k = int(np.searchsorted(model.image_ids, r))
    row_of = {int(p): j for j, p in enumerate(model.point_ids)}
    index = {int(i): j for j, i in enumerate(model.image_ids)}
    C, S = {}, {}
    if mode == "angle":
        edge, w = view_selection.angle_table(*angle)
        assert (np.diff(edge) <= 0).all()
        centers = model.centers()
    for p in model.obs_point[model.img_offset[k]:model.img_offset[k + 1]]:
        if p <= 0:
            continue
        j = row_of[int(p)]
        for s in model.trk_image[model.trk_offset[j]:model.trk_offset[j + 1]]:
            s = int(s)
            C[s] = C.get(s, 0) + 1
            if mode == "angle" and s != r:
                a, b = centers[k] - model.xyz[j], centers[index[s]] - model.xyz[j]
                la, lb = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
                add = 0
                if la != 0.0 and lb != 0.0:
                    add = int(w[_bin_fast(((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (np.sqrt(la) * np.sqrt(lb)), edge)])
                S[s] = S.get(s, 0) + add
    return C, (S if mode == "angle" else C)


def view(model, r, mode="points", angle=view_selection.ANGLE_DEFAULT):
    """{"seen", "max", "sources": [(id, score, count)] in the rule's order} of the image id r."""
    C, S = rows(model, r, mode, angle)
    others = [s for s in C if s != r]
    top = max([S.get(s, 0) for s in others], default=0)
    src = [(s, S.get(s, 0), C[s]) for s in others if C[s] > 10 and 10 * S.get(s, 0) > top]
    return {"seen": sum(1 for s in others if C[s] > 0), "max": top, "sources": sorted(src, key=lambda e: (-e[1], e[0]))}


def select(model, base_size=None, overlap=1, border=None, mode="points", angle=view_selection.ANGLE_DEFAULT):
    """(pairs, block list, scene border) as view_selection.select returns them, by the restatement."""
    block_list, scene = blocks(model, base_size, overlap, border)
    mask = references(model, block_list)
    div = 1024.0 if mode == "angle" else 1.0
    listed = {}
    for k in np.nonzero(mask.any(0))[0]:
        v = view(model, int(model.image_ids[k]), mode, angle)
        if v["seen"] >= 3:
            listed[int(model.image_ids[k])] = [(s, score / div) for s, score, _ in v["sources"]]
    pairs = [(r, listed[r]) for r in sorted(listed)]
    out = []
    for b, rng in enumerate(block_list):
        views = [int(i) for i in model.image_ids[mask[b]] if int(i) in listed]
        if views:
            out.append(([float(x) for x in rng], views))
    return pairs, out, [float(x) for x in scene]


def texts(pairs, block_list, scene):
    """The three files' texts, formatted here (not by the module under test)."""
    vp = ["%d" % len(pairs)]
    for r, src in pairs:
        vp += ["%d" % r, "%d " % len(src) + "".join("%d %.4f " % (s, v) for s, v in src)]
    bl = ["%d" % len(block_list)]
    for rng, views in block_list:
        bl += ["".join("%.4f " % v for v in rng), "".join("%d " % v for v in views)]
    return {"viewpair": "\n".join(vp) + "\n", "blocks": "\n".join(bl) + "\n", "scene_border": "".join(str(v) + "\n" for v in scene)}


# ----------------------------------------------------------------------------------------
# canonical forms of the files
# ----------------------------------------------------------------------------------------
def canonical_pairs(text):
    """viewpair.txt -> {view id: [(score text, sorted ids with it), ...] by score descending}: what does not depend on the
    order of equal scores, nor on the order of the views."""
    lines = text.split("\n")
    out = {}
    for v in range(int(lines[0])):
        w = lines[2 + 2 * v].split()
        assert int(w[0]) == (len(w) - 1) // 2
        groups = {}
        for s, score in zip(w[1::2], w[2::2]):
            groups.setdefault(score, []).append(int(s))
        scores = [float(x) for x in w[2::2]]
        assert scores == sorted(scores, reverse=True)
        assert int(lines[1 + 2 * v]) not in out
        out[int(lines[1 + 2 * v])] = [(k, sorted(groups[k])) for k in sorted(groups, key=float, reverse=True)]
    return out


def canonical_blocks(text):
    """blocks.txt -> [(the six range texts, sorted ids)] in the file's order."""
    lines = text.split("\n")
    return [(lines[1 + 2 * b].split(), sorted(int(x) for x in lines[2 + 2 * b].split())) for b in range(int(lines[0]))]


def golden(scene, name):
    with open(os.path.join(GOLDEN, scene, name)) as f:
        return f.read()
