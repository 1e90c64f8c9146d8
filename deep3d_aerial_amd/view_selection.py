"""View selection and scene blocks from a COLMAP sparse model: the first stage of the pipeline, the one that writes the
`viewpair.txt`, `blocks.txt` and `scene_border.txt` every later stage starts from.  It replaces the
reference's pycolmap/view_selection.py (calculate_block_border, select_view_based_viewed_points in its 'triangulated_points'
mode) and its three writers; the reader of the model is sparse_model.py.

The rule.

* Scene border and blocks: host, fp64, the reference's arithmetic.
  - lo_a, hi_a = np.percentile(a, [0.5, 99.5]) for a = x, y, z over every point of the model.
  - The scene border (x0, x1, y0, y1, z0, z1) is `border` when given, else those six values.
  - The block size (sx, sy, sz) is `base_size` when given, else ((hi_x - lo_x) / 2, (hi_y - lo_y) / 2, hi_z - lo_z).
  - nx = ceil((x1 - x0) / sx) and ny = ceil((y1 - y0) / sy) blocks, row-major: j (y) outside, i (x) inside.
  - Block (i, j) = [bx, bx + sx + o, by, by + sy + o, lo_z, hi_z] with bx = x0 + i sx - o, by = y0 + j sy - o, o the overlap.
  - Two quirks are the reference's and are kept so that blocks.txt agrees with its file: the overlap extends a block on its
    low side only (its high side is x0 + (i + 1) sx), and z always comes from the percentiles, even when `border` is given.
* Reference views of a block: GPU.  Image k belongs to block b iff some point with id > 0 whose track holds k has
  b[0] < x < b[1] and b[2] < y < b[3]: strict comparisons in fp64; z is not tested.
* Score "points" (the default; the reference's 'triangulated_points'): GPU.  For a reference image r,
  C_r[s] = sum over the observations o of r that have a point p of the number of entries of track(p) equal to s.
  Multiplicities count on both sides: a point observed twice by r and named twice by s adds 4, as the reference's `extend` and
  `count` do.  The row's own column C_r[r] is ignored.
  - seen_r = the number of s != r with C_r[s] > 0; r is listed iff seen_r >= 3 (the reference tests len(count_set) > 3 on a
    set that holds r itself).
  - max_r = max over s != r of C_r[s].
  - The sources of r are the s != r with C_r[s] > 10 and 10 C_r[s] > max_r.  The reference writes x > max / 10.0 in fp64: for
    integers below 2^32 the two agree, because 10 x > max means x >= max / 10 + 0.1, far more than the rounding of the
    quotient moves it, and 10 x <= max means x <= max / 10, which a correctly rounded quotient of an exact x keeps.
  - A listed view may have no source: it is still listed, with `0`.
* Score "angle" (opt-in): the baseline-aware score of the usual COLMAP-to-MVSNet converters, made exact.  Beside C, a second
  row S_r[s] = sum over the same (o, track entry) pairs with s != r of W[bin].  Per pair, in fp64 with every operation rounded
  once: a = C_r - X_p, b = C_s - X_p (C the camera centres -R^T t, X_p the point), dot = (a_x b_x + a_y b_y) + a_z b_z,
  c = dot / (sqrt(|a|^2) sqrt(|b|^2)), |a|^2 = (a_x a_x + a_y a_y) + a_z a_z; a zero length gives weight 0.  The table is
  angle_table(theta0, sigma1, sigma2), the single copy: 1800 bins of 0.1 degree, edge[k] = cos(k 0.1 deg),
  W[k] = rint(1024 w((k + 0.5) 0.1 deg)), w(t) = exp(-(t - theta0)^2 / (2 sigma^2)) with sigma = sigma1 for t <= theta0 and
  sigma2 above; defaults 5, 1, 10 degrees.  bin = the largest k in 0 .. 1799 with c <= edge[k]; c > 1 gives bin 0.  The device
  computes no transcendental function: it searches the table it is handed.  Listing goes by seen_r as above; the sources are
  the s != r with C_r[s] > 10 and 10 S_r[s] > max over s != r of S_r; the written score is S / 1024.
* All sums are unsigned 32-bit integers.  An image whose sum over its observations of the track lengths is >= 2^22 is refused
  (ValueError): then no C reaches 2^22 and no S reaches 2^32.
* Order: this project's own, because the reference's is the iteration order of a Python set.  Sources go by score descending,
  then by image id ascending.  Views in viewpair.txt and in a block's list go by image id ascending.  Blocks stay in the
  reference's order; a block with no listed view is dropped; a view listed in several blocks is written once in viewpair.txt.
* Files, in the reference's formats (IO/params_io.py):
  - viewpair.txt: `N`, then per view `id` on a line and `n id score id score ... ` on the next, the score as {:.4f}.
  - blocks.txt: `N`, then per block a line of six {:.4f} values and a line of the ids of its views.
  - scene_border.txt: six lines, str(float) each.
  dataset.read_view_pair_text and dataset.read_scene_blocks read them.

The two GPU parts are HIP (csrc/view_select.hip): one lane per point for the blocks, one workgroup per reference image for the
rows, whose counters live in LDS while they fit (rows * n_img <= lds_images, rows = 1 or 2) and in a scratch of at most 1024
rows otherwise, with identical bits.  Integer atomicAdd only.  The final order of the sources is torch.sort (plumbing).  There
is no CPU fallback.

Out of scope: the reference's 'tie_points' mode (it reads the SQLite match database and has no GPU work), the predef export of
the cameras, `cameras.*`, a cap on the number of sources (the dataset applies view_num), selection sharded over ranks, and any
selection without tie points.

    python -m deep3d_aerial_amd.view_selection --sparse DIR --out BLOCK_FOLDER [--block_size X,Y,Z] [--overlap M]
        [--border Xmin,Xmax,Ymin,Ymax,Zmin,Zmax] [--score points|angle] [--angle T0,S1,S2] [--json LOG.json]
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import _geom, _lib, sparse_model
from ._geom import ptr as _ptr, stream as _stream

MIN_SEEN = 3            # a listed view sees at least this many other images
MIN_COUNT = 10          # a source shares more than this many (observation, track entry) pairs
MAX_PAIRS = 1 << 22     # sum of the track lengths over an image's observations, exclusive
ANGLE_BINS = 1800
ANGLE_SCALE = 1024
ANGLE_DEFAULT = (5.0, 1.0, 10.0)
MODES = ("points", "angle")

load = sparse_model.load


# ----------------------------------------------------------------------------------------
# host: the table, the blocks
# ----------------------------------------------------------------------------------------
def angle_table(theta0=5.0, sigma1=1.0, sigma2=10.0):
    """(edge fp64 [1800], W uint32 [1800]) of the module's docstring.  The only copy of this code: the kernel and the tests'
    restatement both search the table this returns."""
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not (math.isfinite(theta0) and sigma1 > 0 and sigma2 > 0 and math.isfinite(sigma1) and math.isfinite(sigma2)):
        raise ValueError("angle needs a finite theta0 and sigma1, sigma2 > 0 (got %r, %r, %r)" % (theta0, sigma1, sigma2))
    k = np.arange(ANGLE_BINS, dtype=np.float64)
    edge = np.cos(np.deg2rad(k * 0.1))
    mid = (k + 0.5) * 0.1
    sigma = np.where(mid <= theta0, sigma1, sigma2)
    w = np.exp(-((mid - theta0) ** 2) / (2.0 * sigma * sigma))
    return edge, np.rint(ANGLE_SCALE * w).astype(np.uint32)


def scene_blocks(model, base_size=None, overlap=1, border=None):
    """(blocks, scene_border): the list of [x_min, x_max, y_min, y_max, z_min, z_max] of every block, row-major, and the six
    values of the scene border, as Python floats (module docstring)."""
    if model.n_pts == 0:
        raise ValueError("the model has no point: no scene border")
    lo_x, hi_x = np.percentile(model.xyz[:, 0], [0.5, 99.5])
    lo_y, hi_y = np.percentile(model.xyz[:, 1], [0.5, 99.5])
    lo_z, hi_z = np.percentile(model.xyz[:, 2], [0.5, 99.5])
    if border is not None:
        if len(border) != 6:
            raise ValueError("border needs six values (got %d)" % len(border))
        scene = [float(v) for v in border]
    else:
        scene = [float(v) for v in (lo_x, hi_x, lo_y, hi_y, lo_z, hi_z)]
    if base_size is not None:
        if len(base_size) != 3:
            raise ValueError("base_size needs three values (got %d)" % len(base_size))
        size = [float(v) for v in base_size]
    else:
        size = [float((hi_x - lo_x) / 2.0), float((hi_y - lo_y) / 2.0), float((hi_z - lo_z) / 1.0)]
    if not (size[0] > 0 and size[1] > 0 and all(math.isfinite(v) for v in size + scene)):
        raise ValueError("block size %r over border %r: the x and y sizes must be > 0 and everything finite" % (size, scene))
    o = float(overlap)
    nx = math.ceil((scene[1] - scene[0]) / size[0])
    ny = math.ceil((scene[3] - scene[2]) / size[1])
    blocks = []
    for j in range(ny):
        for i in range(nx):
            b = [0.0, 0.0, 0.0, 0.0, float(lo_z), float(hi_z)]
            b[0] = scene[0] + i * size[0] - o
            b[1] = b[0] + size[0] + o
            b[2] = scene[2] + j * size[1] - o
            b[3] = b[2] + size[1] + o
            blocks.append(b)
    return blocks, scene


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------
def max_blocks():
    return int(_lib.CONSTANTS["D3D_VIEW_SELECT_MAX_BLOCKS"])


def lds_images():
    """The counters a workgroup's LDS holds (d3d_view_select_lds_images): the default of score()'s lds_images."""
    return int(_lib.load().d3d_view_select_lds_images())


def _device(model):
    if not isinstance(model, sparse_model.SparseModel):
        raise TypeError("model must be a SparseModel (view_selection.load)")
    if not torch.cuda.is_available():
        raise RuntimeError("views are selected on the GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    cache = model.__dict__.setdefault("_on_device", {})
    if dev not in cache:
        cache[dev] = model.to_device(dev)
    return cache[dev], dev


def block_references(model, blocks):
    """mask uint8 [n_blocks, n_img] on the GPU: mask[b][k] = 1 iff image k (dense index) is a reference view of blocks[b]."""
    blocks = np.asarray(blocks, np.float64).reshape(-1, 6) if len(blocks) else np.zeros((0, 6), np.float64)
    if len(blocks) > max_blocks():
        raise ValueError("%d blocks: at most %d (a larger block size gives fewer)" % (len(blocks), max_blocks()))
    d, dev = _device(model)
    lib = _lib.load()
    n_blocks, n_img = int(blocks.shape[0]), model.n_img
    mask = torch.empty((n_blocks, n_img), dtype=torch.uint8, device=dev)
    if n_blocks == 0 or n_img == 0:
        return mask
    table = torch.from_numpy(np.ascontiguousarray(blocks[:, :4])).to(dev)
    n_trk = int(d["trk_image"].shape[0])
    _lib.check(lib.d3d_view_select_blocks(_ptr(d["xyz"]) if model.n_pts else None, _ptr(d["trk_offset"]), _ptr(d["trk_image"]) if n_trk else None,
                                          model.n_pts, n_trk, d["p_first"], n_img, _ptr(table), n_blocks, _ptr(mask), _stream()),
               "d3d_view_select_blocks")
    return mask


class Scores(object):
    """What score() returns, device tensors: refs int64 [n_ref] (image ids, the caller's order), seen int32 [n_ref],
    max int64 [n_ref] (the largest score over the other images), offset int64 [n_ref + 1], and per source, view by view in
    the order of the rule, src int64 (image ids), score int64 (C, or S in angle mode) and count int64 (C).  host(): the same as
    numpy arrays, in one dict."""

    def __init__(self, mode, refs, seen, max, offset, src, score, count):
        self.mode, self.refs, self.seen, self.max, self.offset, self.src, self.score, self.count = mode, refs, seen, max, offset, src, score, count

    def host(self):
        out = {k: getattr(self, k).cpu().numpy() for k in ("refs", "seen", "max", "offset", "src", "score", "count")}
        out["mode"] = self.mode
        return out


def _mode(mode):
    if mode == "tie_points":
        raise ValueError("mode 'tie_points' is out of scope: it reads the SQLite match database and has no GPU work")
    if mode not in MODES:
        raise ValueError("mode must be one of %r (got %r)" % (MODES, mode))
    return mode


def _rows(model, d, dev, refs_k, seg_d, n_seg, table, lds):
    """One d3d_view_select_rows call: refs_k int32 [n_ref] dense indices and seg_d int64 [n_ref + 1] on the device, table =
    (edge, weight) device tensors for angle mode or None -> (seen, maxv, n_src [n_ref], src, score, count [n_seg]) int32 tensors,
    the unsigned ones as their bits; the segments' tails are not written."""
    lib = _lib.load()
    n_ref, n_img = int(refs_k.shape[0]), model.n_img
    seen = torch.empty((n_ref,), dtype=torch.int32, device=dev)
    maxv = torch.empty((n_ref,), dtype=torch.int32, device=dev)
    n_src = torch.empty((n_ref,), dtype=torch.int32, device=dev)
    src = torch.empty((n_seg,), dtype=torch.int32, device=dev)
    val = torch.empty((n_seg,), dtype=torch.int32, device=dev)
    cnt = torch.empty((n_seg,), dtype=torch.int32, device=dev)
    if n_ref:
        m = 0 if table is None else 1
        scratch, nbytes = _geom.scratch(lib.d3d_view_select_scratch_bytes, n_ref, n_img, m, lds, device=dev)
        edge_d, weight_d = table if m else (None, None)
        n_obs, n_trk = int(d["obs_point"].shape[0]), int(d["trk_image"].shape[0])
        pn = (lambda t, n: _ptr(t) if n else None)
        _lib.check(lib.d3d_view_select_rows(_ptr(d["img_offset"]), pn(d["obs_point"], n_obs), n_obs, _ptr(d["trk_offset"]), pn(d["trk_image"], n_trk),
                                            model.n_pts, n_trk, n_img, _ptr(refs_k), n_ref, m, _ptr(d["centers"]) if m else None,
                                            pn(d["xyz"], model.n_pts) if m else None, _ptr(edge_d), _ptr(weight_d), ANGLE_BINS if m else 0, lds,
                                            _ptr(scratch), nbytes, _ptr(seg_d), n_seg, _ptr(seen), _ptr(maxv), _ptr(n_src), pn(src, n_seg),
                                            pn(val, n_seg), pn(cnt, n_seg), _stream()), "d3d_view_select_rows")
    return seen, maxv, n_src, src, val, cnt


def score(model, refs, mode="points", angle=ANGLE_DEFAULT, lds_images=None):
    """The sources of the reference images `refs` (image ids, any order) -> Scores.  mode "points" | "angle"; angle =
    (theta0, sigma1, sigma2) in degrees; lds_images: the counters to keep in LDS (default and maximum: lds_images()) -- a call
    whose rows need more runs on the scratch path, with the same bits."""
    mode = _mode(mode)
    edge, weight = angle_table(*angle) if mode == "angle" else (None, None)
    refs = np.asarray(refs, np.int64).reshape(-1)
    n_img, n_ref = model.n_img, int(refs.shape[0])
    at = np.minimum(np.searchsorted(model.image_ids, refs), max(n_img - 1, 0))
    if n_ref and (n_img == 0 or (model.image_ids[at] != refs).any()):
        bad = refs if n_img == 0 else refs[model.image_ids[at] != refs]
        raise ValueError("refs names image id %d, which the model does not hold" % bad[0])
    pairs = model.pairs_per_image()
    if n_img and int(pairs.max()) >= MAX_PAIRS:
        k = int(np.argmax(pairs >= MAX_PAIRS))
        raise ValueError("image id %d: its observations' tracks have %d entries in all, at most 2^22 - 1 (the 32-bit sums could wrap)"
                         % (model.image_ids[k], pairs[k]))
    d, dev = _device(model)
    lib = _lib.load()
    most = int(lib.d3d_view_select_lds_images())
    lds = most if lds_images is None else int(lds_images)
    if not 0 <= lds <= most:
        raise ValueError("lds_images must lie in 0 .. %d (got %r)" % (most, lds_images))
    # a source has C > 10, and the C of a row add up to pairs[r]: at most pairs[r] // 11 sources, and never more than n_img - 1
    room = np.minimum(pairs[at] // (MIN_COUNT + 1), max(n_img - 1, 0)).astype(np.int64) if n_ref else np.zeros((0,), np.int64)
    seg = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    n_seg = int(seg[-1])
    if n_seg > sparse_model.MAX_ENTRIES:
        raise ValueError("%d source slots for %d reference images: at most 2^31 - 1 (score fewer images a call)" % (n_seg, n_ref))
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    refs_k, seg_d, room_d = put(at.astype(np.int32)), put(seg), put(room)
    table = (put(edge), put(weight.view(np.int32))) if mode == "angle" else None
    seen, maxv, n_src, src, val, cnt = _rows(model, d, dev, refs_k, seg_d, n_seg, table, lds)
    ids = put(model.image_ids)
    # the written part of every segment, then the rule's order: by view, score descending, image id ascending (plumbing)
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF
    view = torch.repeat_interleave(torch.arange(n_ref, device=dev), room_d)
    found = torch.minimum(n_src.to(torch.int64), room_d)
    keep = (torch.arange(n_seg, device=dev) - seg_d[view]) < found[view]
    view, s, v, c = view[keep], src[keep].to(torch.int64), u32(val[keep]), u32(cnt[keep])
    order = torch.sort(((0xFFFFFFFF - v) << 31) | s).indices
    order = order[torch.sort(view[order], stable=True).indices]
    offset = torch.cat([torch.zeros((1,), dtype=torch.int64, device=dev), torch.cumsum(found, 0)])
    return Scores(mode, put(refs), seen, u32(maxv), offset, ids[s[order]] if n_img else s, v[order], c[order])


# ----------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------
def pair_text(pairs):
    """The text of viewpair.txt for [(id, [(source id, score), ...]), ...]."""
    text = "%d\n" % len(pairs)
    for view, sources in pairs:
        text += "%d\n%d " % (view, len(sources))
        for s, v in sources:
            text += "{} {:.4f} ".format(int(s), v)
        text += "\n"
    return text


def block_text(blocks):
    """The text of blocks.txt for [(six values, [ids]), ...]."""
    text = "%d\n" % len(blocks)
    for rng, views in blocks:
        text += "".join("{:.4f} ".format(v) for v in rng) + "\n"
        text += "".join("%d " % v for v in views) + "\n"
    return text


def border_text(border):
    return "".join(str(float(b)) + "\n" for b in border)


def assemble(image_ids, blocks, mask, scores):
    """(pairs, block list) of the files from the blocks, the host mask [n_blocks, n_img] and score(...).host() of the images
    the mask names (ascending ids): the listing, the order and the dropped blocks of the module's docstring."""
    div = float(ANGLE_SCALE) if scores["mode"] == "angle" else 1.0
    listed = {}
    for i, r in enumerate(scores["refs"].tolist()):
        if scores["seen"][i] >= MIN_SEEN:
            a, b = int(scores["offset"][i]), int(scores["offset"][i + 1])
            listed[r] = [(int(s), float(v) / div) for s, v in zip(scores["src"][a:b], scores["score"][a:b])]
    pairs = [(r, listed[r]) for r in sorted(listed)]
    out = []
    for b, rng in enumerate(blocks):
        views = [int(i) for i in image_ids[np.nonzero(mask[b])[0]] if int(i) in listed]
        if views:
            out.append(([float(v) for v in rng], views))
    return pairs, out


def select(sparse_dir, out_dir, block_size=None, overlap=1, border=None, mode="points", angle=ANGLE_DEFAULT, lds_images=None):
    """Reads the sparse model under sparse_dir, writes viewpair.txt, blocks.txt and scene_border.txt under out_dir and returns
    {"viewpair": pairs, "blocks": block list, "border": six values, "files": the three paths, "images", "points"}."""
    mode = _mode(mode)
    model = load(sparse_dir)
    blocks, scene = scene_blocks(model, block_size, overlap, border)
    mask = block_references(model, blocks).cpu().numpy()
    refs = model.image_ids[mask.any(0)] if len(blocks) else model.image_ids[:0]
    scores = score(model, refs, mode, angle, lds_images).host()
    pairs, block_list = assemble(model.image_ids, blocks, mask, scores)
    os.makedirs(str(out_dir), exist_ok=True)
    files = {name: os.path.join(str(out_dir), name + ".txt") for name in ("viewpair", "blocks", "scene_border")}
    for name, text in (("viewpair", pair_text(pairs)), ("blocks", block_text(block_list)), ("scene_border", border_text(scene))):
        with open(files[name], "w") as f:
            f.write(text)
    return {"viewpair": pairs, "blocks": block_list, "border": scene, "files": files, "images": model.n_img, "points": model.n_pts}


# ----------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------
def _floats(n, flag):
    def parse(text):
        try:
            vals = [float(v) for v in str(text).split(",")]
        except ValueError:
            vals = []
        if len(vals) != n:
            raise argparse.ArgumentTypeError("%s needs %d comma-separated numbers (got %r)" % (flag, n, text))
        return vals
    return parse


def main(argv=None):
    ap = argparse.ArgumentParser(description="view selection and scene blocks from a COLMAP sparse model")
    ap.add_argument("--sparse", required=True, help="the sparse model folder (images and points3D, .bin or .txt)")
    ap.add_argument("--out", required=True, help="the block folder: viewpair.txt, blocks.txt and scene_border.txt go here")
    ap.add_argument("--block_size", type=_floats(3, "--block_size"), default=None, help="X,Y,Z (default: half the scene in x and y)")
    ap.add_argument("--overlap", type=float, default=1.0, help="overlap of the blocks (world units)")
    ap.add_argument("--border", type=_floats(6, "--border"), default=None, help="Xmin,Xmax,Ymin,Ymax,Zmin,Zmax (default: the percentiles)")
    ap.add_argument("--score", choices=MODES, default="points")
    ap.add_argument("--angle", type=_floats(3, "--angle"), default=list(ANGLE_DEFAULT), help="T0,S1,S2 in degrees (--score angle)")
    ap.add_argument("--json", default=None, help="write a log of the run here too (.json)")
    a = ap.parse_args(argv)
    if a.json is not None and not str(a.json).endswith(".json"):
        ap.error("--json must end in .json")
    if not torch.cuda.is_available():
        raise RuntimeError("views are selected on the GPU (no CPU fallback)")
    out = select(a.sparse, a.out, a.block_size, a.overlap, a.border, a.score, tuple(a.angle))
    log = {"sparse": str(a.sparse), "score": a.score, "angle": list(a.angle) if a.score == "angle" else None, "images": out["images"],
           "points": out["points"], "border": out["border"], "blocks": len(out["blocks"]), "views": len(out["viewpair"]),
           "sources": sum(len(s) for _, s in out["viewpair"]), "files": out["files"]}
    line = json.dumps(log)
    if a.json is not None:
        os.makedirs(os.path.dirname(os.path.abspath(str(a.json))), exist_ok=True)
        with open(str(a.json), "w") as f:
            f.write(line + "\n")
    print(line)
    return out


if __name__ == "__main__":
    main()
