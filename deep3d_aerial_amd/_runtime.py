"""Runtime plumbing under the operators of ops.py: everything that is neither a kernel's dispatch nor a weight layout.

The current stream and the argument checks that turn tensors into pointers, the sweep workspace, the dispatch counters, side
streams, the host copy of the depth range, the convolution precision state, and the two weight caches (derived_weight over
_derived_cache; _packed / _packed_fold over _pack_cache) whose packing bodies live in _packing.py.  ops.py imports all of
it by name, so `ops._stream`, `ops.dispatch_counts`, `ops.h16_dtype` ... stay the same objects.
"""
import collections
import ctypes
import threading
import weakref

import torch

from . import _lib
from . import config as _cfg
from ._packing import _pack_fold, _pack_gemm, h16_dtype

# depth modes of the sweep entry points (include/deep3d_planesweep.h)
PER_PLANE, PER_PIXEL, AFFINE = (_lib.CONSTANTS["D3D_DEPTH_" + n] for n in ("PER_PLANE", "PER_PIXEL", "AFFINE"))

# Which kernels served the calls so far: name -> count.  The model-level parity tests clear it, run a forward and assert that
# the production kernels (tile convolutions, fused conv-GRU cell, channel-last volumes, window / ring sweeps) were the ones
# dispatched -- not a fallback that happens to give the same numbers.
dispatch_counts = collections.Counter()

# (device index, stream) -> [slot buffer, next slot]: the GroupNorm statistics arenas of ops.GnStats (msrednet.py reads them)
_gn_arenas = {}

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The HIP stream torch currently queues work on.  torch.cuda.current_stream() builds a Stream object through several
    Python layers (8 us; an AdaMVS view makes 860 launches: tools/host_profile.py); the raw handle is one C call."""
    if _raw_stream is not None and _raw_device is not None:
        return ctypes.c_void_p(_raw_stream(_raw_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------------------
# argument checks: tensor -> device pointer
# ----------------------------------------------------------------------------------------
def _chk(t, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the plane-sweep engine only runs on the GPU (no CPU fallback)"
                           % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have %d dims (got shape %s)" % (name, ndim, tuple(t.shape)))
    return ctypes.c_void_p(t.data_ptr())


def _opt(t, name):
    return None if t is None else _chk(t, name)


def _chk16(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
        raise TypeError("%s must be a contiguous CUDA float16 tensor" % name)
    return ctypes.c_void_p(t.data_ptr())


def _dptr(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.numel() == 2):
        raise TypeError("statistics must be a CUDA float64 pair")
    return ctypes.c_void_p(t.data_ptr())


def _ptr_array(tensors, name):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if _chk(t, "%s[%d]" % (name, i), 3) is not None else None
    return arr


# ----------------------------------------------------------------------------------------
# sweep workspace
# ----------------------------------------------------------------------------------------
_forced = [None]


def _sync_force_path():
    """D3D_FORCE_PATH = direct | tiled (tests, profiling): forwarded to the library's test hook when it changes."""
    want = _cfg.get("D3D_FORCE_PATH")
    if want != _forced[0]:
        code = {"": 0, "auto": 0, "direct": 1, "tiled": 2, "window": 3}.get(want)
        if code is None:
            raise ValueError("D3D_FORCE_PATH must be direct, tiled, window or unset (got %r)" % want)
        _lib.check(_lib.load().d3d_debug_force_path(code), "d3d_debug_force_path")
        _forced[0] = want


def _workspace(n_views, C, D, h, w, elem_bytes, device, mode=PER_PIXEL):
    """Scratch for one sweep call, sized by the library FOR THE CALL'S DEPTH MODE (the window kernel's channel-last copy -- 650 MB
    at the last cascade stage -- serves hypothesis volumes only: (lo, step) maps and per-plane depths do not ask for it) and owned
    by torch's caching allocator: the allocator hands the block back only after the work queued on the current stream (this call)
    has been ordered, so calls never share it."""
    _sync_force_path()
    n = int(_lib.load().d3d_sweep_workspace_bytes_for(n_views, C, D, h, w, elem_bytes, mode))
    if n == 0:
        return None, ctypes.c_void_p(0), 0
    buf = torch.empty((n,), dtype=torch.uint8, device=device)
    return buf, ctypes.c_void_p(buf.data_ptr()), n


# ----------------------------------------------------------------------------------------
# side streams
# ----------------------------------------------------------------------------------------
_side_streams = {}   # (device index, caller stream, owner) -> side streams
_side_lock = threading.Lock()


def side_streams(device, n, owner="ops"):
    """`n` side streams for the forward that runs on the CALLER'S CURRENT stream of `device` -- one set per (device, caller stream,
    owner), created on first use.  Two forwards in flight on different streams (two host threads) therefore never
    share a side stream: their forks / joins do not serialise on each other, the GroupNorm slot arenas (keyed by stream) are
    not shared, and a block the caching allocator frees on a side stream is reused behind THAT caller's next fork only."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, owner)
    with _side_lock:
        side = _side_streams.get(key)
        if side is None or len(side) < n:
            side = _side_streams[key] = [torch.cuda.Stream(device) for _ in range(n)]
    return side[:n]


def hand_over(outs, stream):
    """Tensors produced on a side stream and consumed on `stream` from now on: tell the caching allocator (record_stream), so
    that their blocks -- allocated in the side stream's pool -- are not handed out again on the side stream while `stream` still
    reads them.  Walks lists / tuples / dicts.  (Ordering is the join event's job; this is the allocator's bookkeeping.)"""
    if isinstance(outs, torch.Tensor):
        if outs.is_cuda and not _cfg.off("hand_over"):
            outs.record_stream(stream)
    elif isinstance(outs, (list, tuple)):
        for o in outs:
            hand_over(o, stream)
    elif isinstance(outs, dict):
        for o in outs.values():
            hand_over(o, stream)


def on_streams(thunks, device, switch):
    """[f() for f in thunks] with the INDEPENDENT pieces of work going round-robin over the caller's stream and two side streams
    (fork event before, one join event per side piece after): chains of small launches that leave most of the chip idle overlap.
    Same kernels, same operands; `switch` (a key of config.KERNELS) in D3D_KERNELS_OFF keeps everything on the caller's stream.
    The side streams belong to the caller's stream (side_streams), and what the side pieces return is handed over to it."""
    if len(thunks) < 2 or device.type != "cuda" or _cfg.off(switch):
        return [f() for f in thunks]
    main = torch.cuda.current_stream(device)
    side = side_streams(device, 2)
    fork = main.record_event()
    outs, joins = [], []
    for i, f in enumerate(thunks):
        st = (None, side[0], side[1])[i % 3]
        if st is None:
            outs.append(f())
            continue
        with torch.cuda.stream(st):
            st.wait_event(fork)
            outs.append(f())
            joins.append(st.record_event())
        hand_over(outs[-1], main)
    for e in joins:
        main.wait_event(e)
    return outs


# ----------------------------------------------------------------------------------------
# The drivers need the depth range (depth_values[0, 0], depth_values[0, -1]) as host numbers (adamvs.py:565-566 and its siblings
# read it with .item()): on a device tensor that is a device -> host copy, i.e. the host waits for every kernel of the PREVIOUS
# view before it launches the first one of this view.  A caller that built the tensor from host data says so once
# (note_depth_range: predict_views, bench.py) and the forward then never touches the device for it.
# ----------------------------------------------------------------------------------------
_depth_ranges = {}


def note_depth_range(depth_values, dmin, dmax):
    """`depth_values` (a device tensor about to be passed to an Infer_* forward) holds [dmin .. dmax] in its first row: keep the
    host copy of the two numbers (until the tensor is written to or dies)."""
    key = id(depth_values)
    ref = weakref.ref(depth_values, lambda _r, key=key: _depth_ranges.pop(key, None))
    _depth_ranges[key] = (ref, depth_values._version, float(dmin), float(dmax))
    return depth_values


def depth_range_host(depth_values):
    """(dmin, dmax) of an Infer_* forward's depth_values [B,2] | [B,D] as host floats: the noted pair if the caller left one
    (no device access), else read from the tensor (one host sync)."""
    hit = _depth_ranges.get(id(depth_values))
    if hit is not None and hit[0]() is depth_values and hit[1] == depth_values._version:
        return hit[2], hit[3]
    dmin, dmax = (float(v) for v in depth_values[0, [0, -1]].tolist())
    return dmin, dmax


# ----------------------------------------------------------------------------------------
# convolution precision (per thread: config.state)
# ----------------------------------------------------------------------------------------
H16_NAMES = ("h16", "f16", "bf16")


def _norm_precision(mode):
    """"h16" is the fast mode in whatever 16-bit format the library was built with; "f16" / "bf16" name a format and are
    accepted only when the loaded library IS that format -- asking an f16 build for bf16 must not silently run f16."""
    if mode in (None, "fp32", "h16"):
        return mode
    if mode in ("f16", "bf16"):
        if _lib.h16_format() != mode:
            raise ValueError("precision %r asked of a library whose 16-bit operand format is %r (d3d_h16_format; rebuild with "
                             "`make -C deep3d_aerial_amd/csrc H16=%s` or ask for 'h16')" % (mode, _lib.h16_format(), mode))
        return "h16"
    raise ValueError("precision must be 'fp32' or 'h16' (or the library's format by name: %r)" % _lib.h16_format())


def set_conv_precision(mode):
    """"fp32" (default; fp32 accuracy: exact fp32 MFMA or split bf16x3 operands) or "h16" (16-bit matrix-core operands in the
    library's format -- IEEE half unless built otherwise, see _lib.h16_format() -- with fp32 accumulation: BASELINE config 3's
    fast mode) for the regularisers' convolutions.  None = follow the switch table (D3D_CONV_PRECISION).
    PER THREAD (config.state is a threading.local): a forward run in a worker thread follows the switch table's
    D3D_CONV_PRECISION unless that thread calls this itself; to change the process-wide default set
    config.switches["D3D_CONV_PRECISION"]."""
    _cfg.state.conv_precision = _norm_precision(mode)


def conv_precision():
    return _cfg.state.conv_precision or _norm_precision(_cfg.get("D3D_CONV_PRECISION"))


class fp32_convs:
    """Context manager: exact fp32 convolutions inside, whatever the global precision (feature pyramids)."""

    def __enter__(self):
        self.saved = _cfg.state.conv_precision
        _cfg.state.conv_precision = "fp32"

    def __exit__(self, *exc):
        _cfg.state.conv_precision = self.saved
        return False


class h16_convs(fp32_convs):
    """Context manager: 16-bit matrix-core operands inside (BASELINE config 3's fast mode), whatever the global precision."""

    def __enter__(self):
        self.saved = _cfg.state.conv_precision
        _cfg.state.conv_precision = "h16"


def _use_mfma():
    return _cfg.get("D3D_CONV") != "direct"


# ----------------------------------------------------------------------------------------
# The two weight caches.  Entries are keyed by the tensor OBJECT (weak), validated by storage address and in-place version
# counter: load_state_dict / copy_ / optimizer steps bump the version; writes through `.data` do not -- call
# clear_weight_cache() after those.  Captured graphs bake the device pointers of cached tensors, so an entry's lifetime is
# behaviour: two dictionaries, each cleared whole when it passes 4096 entries.
# ----------------------------------------------------------------------------------------
_derived_cache = {}   # (id(weight), tag) -> derived_weight's tensors; tags are shared across call sites on purpose
_pack_cache = {}      # (id(weight), transposed) | (id(weight), "fold", transposed, stride) -> _packed's / _packed_fold's operands


def publish_prepared(weight):
    """A freshly prepared (packed / folded) operand goes into a cache that EVERY stream reads: the forwards run some layers on
    side streams (feature pyramids, RED-Net's conv-GRU levels), so the stream that prepared it waits for the preparation once --
    a cache miss happens at the first forward after a weight changes -- and whoever finds the entry later finds finished data."""
    if isinstance(weight, torch.Tensor) and weight.is_cuda:
        torch.cuda.current_stream(weight.device).synchronize()


def _cached(cache, key, weight, make):
    """cache[key] if it was made from this version of `weight`, else make(weight.detach()) -- published, then stored."""
    hit = cache.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == (weight.data_ptr(), weight._version):
        return hit[2]
    with torch.no_grad():
        out = make(weight.detach())
    publish_prepared(weight)
    if len(cache) > 4096:
        cache.clear()
    cache[key] = (weakref.ref(weight), (weight.data_ptr(), weight._version), out)
    return out


def derived_weight(weight, tag, fn):
    """A tensor computed from a parameter (negated / flipped / re-laid-out weights), cached per parameter
    version like the packed GEMM operands; host-side weight preparation, not data-path arithmetic."""
    def make(w):
        out = fn(w)
        return tuple(t.contiguous() for t in out) if isinstance(out, tuple) else out.contiguous()
    return _cached(_derived_cache, (id(weight), tag), weight, make)


def _packed(weight, transposed):
    """Packed GEMM operands of a k=3 conv weight (_packing._pack_gemm), cached per parameter version."""
    return _cached(_pack_cache, (id(weight), transposed), weight, lambda w: _pack_gemm(w, transposed))


def _packed_fold(weight, transposed, stride):
    """List of launches [(wpack, taps, T, M, mpad, geom tail)] for one layer (_packing._pack_fold), cached like _packed."""
    return _cached(_pack_cache, (id(weight), "fold", transposed, stride), weight, lambda w: _pack_fold(w, transposed, stride))


def clear_weight_cache():
    """Drop every packed / derived weight entry (needed only after writing weights through `.data`)."""
    _pack_cache.clear()
    _derived_cache.clear()
