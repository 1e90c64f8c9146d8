"""Reader of a COLMAP sparse model folder: `images` and `points3D`, in the text form (.txt) or the binary form (.bin)
(DESIGN.md §4.32).  Written from COLMAP's published format description; `cameras.*` is not needed by the view selection and
is not read.

The form is detected per file by which file exists; when both `NAME.bin` and `NAME.txt` are present the binary one is read
(COLMAP itself writes binary by default, and the text form rounds nothing but is slower to parse).

The formats, little-endian where binary:

* images.txt: lines starting with `#` are comments.  Two lines an image: `IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME`, then
  `X Y POINT3D_ID` repeated, one triple per 2-D point (the line may be empty).  POINT3D_ID -1: the 2-D point has no 3-D point.
* images.bin: uint64 count; per image int32 id, 4 doubles qvec, 3 doubles tvec, int32 camera id, the name as bytes up to a 0
  byte, uint64 number of 2-D points, then per 2-D point double x, double y, int64 point id.
* points3D.txt: one line a point: `POINT3D_ID X Y Z R G B ERROR` then `IMAGE_ID POINT2D_IDX` repeated, one pair per track entry.
* points3D.bin: uint64 count; per point uint64 id, 3 doubles xyz, 3 uint8 rgb, double error, uint64 track length, then per
  entry int32 image id, int32 index of the 2-D point.

The record (SparseModel), plain numpy arrays:

* image_ids int64 [n_img] ascending: the position k of an id is the image's dense index; qvec [n_img,4] and tvec [n_img,3]
  fp64 (world to camera, qvec = w x y z); names, a list.
* the observations as CSR by image: img_offset int64 [n_img+1], obs_point int64 [n_obs] = the point ids in the file's order
  (-1, or any id <= 0: no point).
* point_ids int64 [n_pts] ascending: the position p of an id is the point's dense index; xyz fp64 [n_pts,3].
* the tracks as CSR by point: trk_offset int64 [n_pts+1], trk_image int64 [n_trk] = the image ids in the file's order.

Refused with a ValueError that names the id: an observation whose point id is > 0 and absent from points3D; a track that names
an unknown image; an image or point id given twice; more than 2^31 - 1 observations or track entries; a truncated file.
Points with an id <= 0 take no part in the selection (no observation can name them) but stay in the record: the scene border
is the percentile of every point read, as the reference's is.
"""
import os
import struct

import numpy as np

MAX_ENTRIES = (1 << 31) - 1


class SparseModel(object):
    """The record of the module's docstring.  centers(): the camera centres; to_device(): the dense-index device form."""

    def __init__(self, image_ids, qvec, tvec, names, img_offset, obs_point, point_ids, xyz, trk_offset, trk_image):
        self.image_ids, self.qvec, self.tvec, self.names = image_ids, qvec, tvec, names
        self.img_offset, self.obs_point = img_offset, obs_point
        self.point_ids, self.xyz = point_ids, xyz
        self.trk_offset, self.trk_image = trk_offset, trk_image

    n_img = property(lambda self: int(self.image_ids.shape[0]))
    n_pts = property(lambda self: int(self.point_ids.shape[0]))

    def centers(self):
        """C = -R^T t per image, [n_img,3] fp64: R from the quaternion (w, x, y, z) as given (COLMAP stores unit quaternions), every
        component summed left to right."""
        w, x, y, z = (self.qvec[:, k] for k in range(4))
        R = np.zeros((self.n_img, 3, 3), np.float64)
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y
        t = self.tvec
        return np.stack([-((R[:, 0, k] * t[:, 0] + R[:, 1, k] * t[:, 1]) + R[:, 2, k] * t[:, 2]) for k in range(3)], 1)

    def dense(self):
        """(obs_p int32 [n_obs], trk_k int32 [n_trk], p_first): obs_point as dense point indices (-1: no point), trk_image as
        dense image indices, and the number of points with an id <= 0 (they come first).  Checked when the model was read; computed
        once (the record's arrays are not meant to be changed)."""
        if "_dense" in self.__dict__:
            return self._dense
        obs_p = np.full(self.obs_point.shape, -1, np.int32)
        has = self.obs_point > 0
        obs_p[has] = np.searchsorted(self.point_ids, self.obs_point[has]).astype(np.int32)
        trk_k = np.searchsorted(self.image_ids, self.trk_image).astype(np.int32)
        self._dense = (obs_p, trk_k, int(np.searchsorted(self.point_ids, 0, side="right")))
        return self._dense

    def pairs_per_image(self):
        """int64 [n_img]: the sum over an image's observations with a point of the length of that point's track.  Computed once."""
        if "_pairs" in self.__dict__:
            return self._pairs
        obs_p = self.dense()[0]
        length = np.diff(self.trk_offset)
        per_obs = np.where(obs_p >= 0, length[np.maximum(obs_p, 0)] if self.n_pts else 0, 0).astype(np.int64)
        cum = np.concatenate([[0], np.cumsum(per_obs)]).astype(np.int64)
        self._pairs = cum[self.img_offset[1:]] - cum[self.img_offset[:-1]]
        return self._pairs

    def to_device(self, device="cuda"):
        """{"img_offset" int64, "obs_point" int32, "trk_offset" int64, "trk_image" int32, "xyz" fp64, "centers" fp64} as
        tensors on `device`, in dense indices, and "p_first" (an int)."""
        import torch

        obs_p, trk_k, p_first = self.dense()
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return {"img_offset": put(self.img_offset), "obs_point": put(obs_p), "trk_offset": put(self.trk_offset), "trk_image": put(trk_k),
                "xyz": put(self.xyz), "centers": put(self.centers()), "p_first": p_first}


def _count(n, what, path):
    if n > MAX_ENTRIES:
        raise ValueError("%s: %d %s, at most 2^31 - 1" % (path, n, what))


class _Bytes(object):
    """A cursor over a binary file's bytes; a read past the end is a ValueError that names what was being read."""

    def __init__(self, path):
        with open(path, "rb") as f:
            self.data = f.read()
        self.path, self.at = path, 0

    def take(self, fmt, what):
        size = struct.calcsize(fmt)
        if self.at + size > len(self.data):
            raise ValueError("%s is truncated: %s needs %d bytes at offset %d of %d" % (self.path, what, size, self.at, len(self.data)))
        out = struct.unpack_from(fmt, self.data, self.at)
        self.at += size
        return out

    def array(self, dtype, n, what):
        size = np.dtype(dtype).itemsize * n
        if self.at + size > len(self.data):
            raise ValueError("%s is truncated: %s needs %d bytes at offset %d of %d" % (self.path, what, size, self.at, len(self.data)))
        out = np.frombuffer(self.data, dtype, count=n, offset=self.at)
        self.at += size
        return out


def _images_bin(path):
    b = _Bytes(path)
    n, = b.take("<Q", "the image count")
    ids, q, t, names, obs = [], [], [], [], []
    total = 0
    for k in range(n):
        rec = b.take("<i7di", "image %d of %d" % (k + 1, n))
        end = b.data.find(b"\0", b.at)
        if end < 0:
            raise ValueError("%s is truncated: the name of image id %d has no end" % (path, rec[0]))
        names.append(b.data[b.at:end].decode("utf-8", "replace"))
        b.at = end + 1
        m, = b.take("<Q", "the number of 2-D points of image id %d" % rec[0])
        total += m
        _count(total, "observations", path)
        pts = b.array(np.dtype([("x", "<f8"), ("y", "<f8"), ("p", "<i8")]), m, "the 2-D points of image id %d" % rec[0])
        ids.append(rec[0])
        q.append(rec[1:5])
        t.append(rec[5:8])
        obs.append(pts["p"].astype(np.int64))
    return ids, q, t, names, obs


def _images_txt(path):
    ids, q, t, names, obs = [], [], [], [], []
    total = 0
    with open(path) as f:
        while True:
            line = f.readline()
            if not line:
                break
            line = line.strip()
            if not line or line[0] == "#":
                continue
            w = line.split()
            try:
                if len(w) < 10:
                    raise ValueError
                image_id, vals = int(w[0]), [float(v) for v in w[1:8]]
            except ValueError:
                raise ValueError("%s: cannot read the image line %r" % (path, line[:80]))
            second = f.readline()
            if not second:
                raise ValueError("%s is truncated: image id %d has no line of 2-D points" % (path, image_id))
            e = second.split()
            try:
                if len(e) % 3:
                    raise ValueError
                pts = np.array([int(v) for v in e[2::3]], np.int64)
            except ValueError:
                raise ValueError("%s is truncated: the 2-D points of image id %d are not whole X Y POINT3D_ID triples" % (path, image_id))
            total += len(pts)
            _count(total, "observations", path)
            ids.append(image_id)
            q.append(vals[:4])
            t.append(vals[4:])
            names.append(" ".join(w[9:]))
            obs.append(pts)
    return ids, q, t, names, obs


def _points_bin(path):
    b = _Bytes(path)
    n, = b.take("<Q", "the point count")
    ids, xyz, trk = [], [], []
    total = 0
    for k in range(n):
        rec = b.take("<Q3d3Bd", "point %d of %d" % (k + 1, n))
        pid = rec[0] if rec[0] < 1 << 63 else rec[0] - (1 << 64)
        m, = b.take("<Q", "the track length of point id %d" % pid)
        total += m
        _count(total, "track entries", path)
        ids.append(pid)
        xyz.append(rec[1:4])
        trk.append(b.array("<i4", 2 * m, "the track of point id %d" % pid)[0::2].astype(np.int64))
    return ids, xyz, trk


def _points_txt(path):
    ids, xyz, trk = [], [], []
    total = 0
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line[0] == "#":
                continue
            w = line.split()
            try:
                if len(w) < 8:
                    raise ValueError
                pid, pos = int(w[0]), [float(v) for v in w[1:4]]
            except ValueError:
                raise ValueError("%s is truncated: cannot read the point line %r" % (path, line[:80]))
            try:
                if len(w) % 2:
                    raise ValueError
                track = np.array([int(v) for v in w[8::2]], np.int64)
            except ValueError:
                raise ValueError("%s is truncated: the track of point id %d is not whole IMAGE_ID POINT2D_IDX pairs" % (path, pid))
            total += len(track)
            _count(total, "track entries", path)
            ids.append(pid)
            xyz.append(pos)
            trk.append(track)
    return ids, xyz, trk


def _csr(order, lists):
    lengths = np.array([len(lists[k]) for k in order], np.int64)
    offset = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flat = np.concatenate([lists[k] for k in order]).astype(np.int64) if len(order) and offset[-1] else np.zeros((0,), np.int64)
    return offset, flat


def _pick(folder, name):
    for ext, form in ((".bin", "bin"), (".txt", "txt")):
        path = os.path.join(str(folder), name + ext)
        if os.path.exists(path):
            return path, form
    raise FileNotFoundError("neither %s.bin nor %s.txt under %s" % (name, name, folder))


def load(folder):
    """The SparseModel of a sparse model folder (module docstring): images.{bin,txt} and points3D.{bin,txt}, the binary form
    preferred where both exist."""
    ipath, iform = _pick(folder, "images")
    ppath, pform = _pick(folder, "points3D")
    ids, q, t, names, obs = (_images_bin if iform == "bin" else _images_txt)(ipath)
    pids, xyz, trk = (_points_bin if pform == "bin" else _points_txt)(ppath)
    ids, pids = np.array(ids, np.int64).reshape(-1), np.array(pids, np.int64).reshape(-1)
    order, porder = np.argsort(ids, kind="stable"), np.argsort(pids, kind="stable")
    image_ids, point_ids = ids[order], pids[porder]
    dup = np.nonzero(np.diff(image_ids) == 0)[0]
    if dup.size:
        raise ValueError("%s: image id %d is given twice" % (ipath, image_ids[dup[0]]))
    dup = np.nonzero(np.diff(point_ids) == 0)[0]
    if dup.size:
        raise ValueError("%s: point id %d is given twice" % (ppath, point_ids[dup[0]]))
    img_offset, obs_point = _csr(order, obs)
    trk_offset, trk_image = _csr(porder, trk)
    # every observation with a point names a point that exists
    has = np.nonzero(obs_point > 0)[0]
    at = np.minimum(np.searchsorted(point_ids, obs_point[has]), max(len(point_ids) - 1, 0))
    bad = has[point_ids[at] != obs_point[has]] if len(point_ids) else has
    if bad.size:
        k = int(np.searchsorted(img_offset, bad[0], side="right")) - 1
        raise ValueError("%s: image id %d observes point id %d, which %s does not hold" % (ipath, image_ids[k], obs_point[bad[0]], ppath))
    # every track entry names an image that exists
    at = np.minimum(np.searchsorted(image_ids, trk_image), max(len(image_ids) - 1, 0))
    bad = np.nonzero(image_ids[at] != trk_image)[0] if len(image_ids) else np.arange(len(trk_image))
    if bad.size:
        p = int(np.searchsorted(trk_offset, bad[0], side="right")) - 1
        raise ValueError("%s: the track of point id %d names image id %d, which %s does not hold" % (ppath, point_ids[p], trk_image[bad[0]], ipath))
    f64 = lambda rows, width, o: np.array([rows[k] for k in o], np.float64).reshape(-1, width)
    return SparseModel(image_ids, f64(q, 4, order), f64(t, 3, order), [names[k] for k in order], img_offset, obs_point, point_ids,
                       f64(xyz, 3, porder), trk_offset, trk_image)
