"""What the stage benches (cloud_bench, cloud_compare_bench, cloud_outliers_bench, mesh_compare_bench, dtm_bench, objects_bench,
outlines_bench, ortho_mesh_bench, ...) share: device-event timing of a call, the median / min / max of the times with the bytes
a kernel must move as a time at 8 TB/s, and a second build of the library bound with the header's signatures.  Not a tool."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deep3d_aerial_amd import _lib  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def timed(call, runs):
    """The ms of `runs` calls, each on its own pair of device events, after one warm-up call."""
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms, nbytes=None):
    med = float(np.median(ms))
    r = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if nbytes is not None:
        floor = nbytes / PEAK_BYTES_PER_S * 1e3
        r.update(bytes=int(nbytes), ms_at_8TBps=round(floor, 4), share_of_8TBps=round(floor / med, 4) if med > 0 else None)
    return r


def bind(path):
    """Another build of the library with the header's signatures."""
    lib = ctypes.CDLL(path)
    for name, sig in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, ctypes.c_int)
    return lib
