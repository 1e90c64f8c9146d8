"""What the geometry stages (dsm, ortho, mesh, texture, fuse) share on the host: pointers, the stream, scratch buffers, record
tables, view batches, the checks of a mesh's arrays and the camera of a view.  Internal: the stages re-export what callers use."""
import contextlib
import ctypes
import math
import os
import time

import numpy as np
import torch


def stream():
    from . import ops

    return ops._stream()


def ptr(t):
    """The device pointer of a tensor as a void pointer; None is the null pointer."""
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def scratch(lib_fn, *args, device):
    """(uint8 tensor on `device`, byte count) for a d3d_*_scratch_bytes function and its arguments; a count of 0 (the
    function refused the sizes) still gets a 1-byte tensor, so the pointer is never null."""
    nbytes = int(lib_fn(*args))
    return torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=device), nbytes


def records(struct_array, device):
    """A ctypes array of records in device memory (one host-to-device copy, ordered on the current stream)."""
    return torch.frombuffer(bytearray(bytes(struct_array)), dtype=torch.uint8).to(device)


@contextlib.contextmanager
def timed(timings, key, start=False, always=True):
    """The seconds the block takes into timings[key], when timings (a dict) is given.  The device is synchronised when the block
    ends, and with start=True before it begins as well; with always=False only when timings is given.  A block that raises is
    neither synchronised nor timed."""
    sync = always or timings is not None
    if start and sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    if sync:
        torch.cuda.synchronize()
    if timings is not None:
        timings[key] = time.perf_counter() - t0


def is_real(x, above=None, at_least=None):
    """x is a finite real number -- an int, a float or a numpy scalar of either kind, never a bool -- that lies above `above`
    and at or above `at_least` where they are given.  The caller raises, in its own words."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x):
        return False
    return (above is None or x > above) and (at_least is None or x >= at_least)


def is_int(x, lo, hi=None):
    """x is an integer -- an int or a numpy integer, never a bool -- in lo .. hi (hi None: no upper end)."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        return False
    return lo <= int(x) and (hi is None or int(x) <= hi)


def host(t):
    """A tensor or anything array-like as a host array."""
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def write_bytes(path, data):
    """data written to path, whose folder is made first."""
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(str(path), "wb") as f:
        f.write(data)


PLY_TYPES = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<i4": "int"}   # dtype.str of a record's field -> PLY scalar type


def record_ply_bytes(comment, rec):
    """The bytes of a binary little-endian PLY whose only element is the vertex: one vertex per record of the structured array
    rec, one scalar property per field, named and typed by rec's dtype, in its order."""
    dt = rec.dtype
    head = ["ply", "format binary_little_endian 1.0", "comment %s" % comment, "element vertex %d" % rec.shape[0]]
    head += ["property %s %s" % (PLY_TYPES[dt[f].str], f) for f in dt.names]
    return ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + rec.tobytes()


def check_views_per_batch(views_per_batch):
    if views_per_batch is not None and int(views_per_batch) < 1:
        raise ValueError("views_per_batch must be >= 1 (got %r)" % (views_per_batch,))
    return None if views_per_batch is None else int(views_per_batch)


def batches(views, views_per_batch):
    n = views_per_batch or max(len(views), 1)
    return [views[k:k + n] for k in range(0, len(views), n)]


def check_tensor(t, name, dtype, shape, device, other):
    """t is a contiguous tensor of `dtype` and `shape` on `device`, the device of `other` ("the height", "the mesh")."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
        raise ValueError("%s must be a contiguous %s tensor of shape %s" % (name, dtype, shape))
    if t.device != device:
        raise RuntimeError("%s is on %s, %s on %s (no CPU fallback)" % (name, t.device, other, device))


def check_raster(t, name, dtypes, cells, cells_text, runs):
    """(H, W) of a device raster, checked: ValueError for a wrong shape or dtype or for W * H >= cells (cells_text: the bound as
    the message gives it), the package's error for a CPU tensor; runs: what the stage does on the GPU, in its own words."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dim() != 2 or t.dtype not in dtypes or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be a non-empty [H,W] %s raster (got %s %s)"
                         % (name, " or ".join(str(d).replace("torch.", "") for d in dtypes), tuple(t.shape), t.dtype))
    if t.shape[0] * t.shape[1] >= cells:
        raise ValueError("%s: %d x %d: W * H must stay below %s" % (name, t.shape[1], t.shape[0], cells_text))
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: %s on the GPU (no CPU fallback)" % (name, t.device, runs))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return int(t.shape[0]), int(t.shape[1])


def mesh_arrays(vertices, faces, index_factor, what):
    """(vertices, faces, n, m) contiguous and checked: [n,3] fp32 and [m,3] int32 on one GPU, index_factor * m < 2^31, every
    index in range.  what: the verb of the stage ("cleaned", "textured") for the error text."""
    if not (isinstance(vertices, torch.Tensor) and isinstance(faces, torch.Tensor)):
        raise TypeError("vertices and faces must be tensors")
    if vertices.device.type != "cuda" or faces.device != vertices.device:
        raise RuntimeError("the mesh is %s on the GPU (no CPU fallback); got %s and %s" % (what, vertices.device, faces.device))
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be [n,3] float32 (got %s %s)" % (tuple(vertices.shape), vertices.dtype))
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be [m,3] int32 (got %s %s)" % (tuple(faces.shape), faces.dtype))
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    if n >= 1 << 31 or index_factor * m >= 1 << 31:
        raise ValueError("%d vertices, %d faces: at most 2^31 - 1 vertices and %d m < 2^31" % (n, m, index_factor))
    if m and (int(faces.min()) < 0 or int(faces.max()) >= n):
        raise ValueError("a face index lies outside 0 .. %d" % (n - 1))
    return vertices.contiguous(), faces.contiguous(), n, m


def mvs_cameras(mvs_folder):
    """(name, cam, location, image path) of every {name}_init.pfm + {name}.txt predict wrote under mvs_folder, by name."""
    from . import predict

    names = sorted(f[:-len("_init.pfm")] for f in os.listdir(mvs_folder) if f.endswith("_init.pfm"))
    if not names:
        raise FileNotFoundError("no {name}_init.pfm under %s" % mvs_folder)
    return [(name,) + tuple(predict.read_red_cam(os.path.join(mvs_folder, name + ".txt"))) for name in names]


def load_map(mvs_folder, name, suffix, device):
    """{name}{suffix}.pfm under mvs_folder as a device tensor."""
    from . import predict

    data, _ = predict.load_pfm(os.path.join(mvs_folder, name + suffix + ".pfm"))
    return torch.from_numpy(np.ascontiguousarray(data)).to(device)


def camera_center(R, t):
    """C = -R^T t in fp64, each component summed left to right."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    return np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)], np.float64)


class Camera(object):
    """The camera of a view: K [3,3] and E = Tcw [4,4] (host arrays, used in fp64) split into K, R, t.  A derived class sets
    W and H once it knows the image size; fill() writes R, t, K, W, H of a d3d_*_view_t record.  MeshView derives from this
    class directly: d3d_mesh_view_t has neither an id nor a centre."""

    def __init__(self, K, E):
        K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
        if K.shape != (3, 3) or E.shape != (4, 4):
            raise ValueError("K must be [3,3] and E [4,4] (got %s, %s)" % (K.shape, E.shape))
        self.K, self.R, self.t = K.copy(), E[:3, :3].copy(), E[:3, 3].copy()

    def fill(self, r):
        r.R[:] = list(self.R.ravel())
        r.t[:] = list(self.t)
        r.K[:] = list(self.K.ravel())
        r.W, r.H = self.W, self.H
        return r


class IdCamera(Camera):
    """A camera with the view's id and its centre C: what d3d_ortho_view_t holds beside the maps (OrthoView, texture.Camera)."""

    def __init__(self, id, K, E):
        Camera.__init__(self, K, E)
        self.id = int(id)
        self.C = camera_center(self.R, self.t)

    def fill(self, r):
        Camera.fill(self, r)
        r.C[:] = list(self.C)
        r.id = self.id
        return r
