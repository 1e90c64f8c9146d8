"""Poison what `torch.empty` and its kin return, so a test can ask whether a result depends on what its buffers held before.

A plain helper module: `tests/test_poison.py` and `tests/test_uninitialised_gpu.py` import it, nothing else does.

    with poisoned(0xFF) as log:
        out = stage(...)
    assert log

For the duration `torch.empty`, `torch.empty_like`, `torch.empty_strided` and `torch.Tensor.new_empty` are replaced by wrappers
that call the real function and then set every byte of the new tensor's storage to `byte`.  The fill is an ordinary
`fill_` on a uint8 alias of the storage: on a device tensor it is queued on the current stream, so it is ordered before the
kernel the buffer is handed to.  While the current stream is capturing nothing is filled (a fill would become a node of the
captured graph), and zero-element tensors are skipped; neither is logged.

    byte   fp32 / fp64                 fp16   bf16               int32 / int64        uint8
    0x00   0                           0      0                  0                    0
    0xFF   NaN                         NaN    NaN                -1                   255
    0x7F   3.39e38 / 1.4e306 (finite)  NaN    3.39e38 (finite)   2139062143 / 9.2e18  127

(0x7F7F has an all-ones exponent in fp16 but not in bf16, whose 8 exponent bits are fp32's: in a build whose 16-bit format is
bf16 the 0x7F pattern is the large finite value there too.)

The log is a list with one extra attribute, `on_device`: how many of its entries were tensors in device memory -- a test of
the library asserts on that, since host-side constructors (nn.Module parameters) also come through torch.empty.
"""
import contextlib

import torch

PATTERNS = (0x00, 0xFF, 0x7F)

# (owner, attribute): every allocation route the package uses that leaves memory unwritten (test_poison.py walks the package
# and fails on a route that is not listed here)
WRAPPED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))


def _fill(real_empty, t, byte):
    """Set every byte of `t`'s storage to `byte`; False if nothing was filled."""
    if not isinstance(t, torch.Tensor) or t.numel() == 0:
        return False
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    st = t.untyped_storage()
    with torch.no_grad():
        # a fresh tensor owns its storage, so the alias covers exactly it (a strided one's gaps included)
        raw = real_empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),), (1,))
        raw.fill_(byte)
    return True


class PoisonLog(list):
    """[(function, shape, dtype)] of the tensors filled; on_device counts those in device memory."""
    on_device = 0


def _wrap(name, real, real_empty, byte, log):
    def wrapper(*args, **kwargs):
        t = real(*args, **kwargs)
        if _fill(real_empty, t, byte):
            log.append((name, tuple(t.shape), t.dtype))
            log.on_device += int(t.is_cuda)
        return t

    wrapper.__name__ = name
    wrapper.__wrapped__ = real
    return wrapper


@contextlib.contextmanager
def poisoned(byte):
    """Context manager: every tensor the four functions return inside is pre-filled with `byte`; yields the log, a list of
    (function name, shape, dtype), one entry per tensor filled.  The originals are restored on exit, after an exception too."""
    byte = int(byte)
    if not 0 <= byte <= 0xFF:
        raise ValueError("byte must be in 0..255")
    log = PoisonLog()
    real = [(owner, name, getattr(owner, name)) for owner, name in WRAPPED]
    real_empty = torch.empty
    try:
        for owner, name, fn in real:
            setattr(owner, name, _wrap(name, fn, real_empty, byte, log))
        yield log
    finally:
        for owner, name, fn in real:
            setattr(owner, name, fn)


def raw_equal(a, b):
    """Bit equality of two tensors (shape, dtype and bytes), so that NaNs count."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.bool:
        return bool(torch.equal(a, b))
    return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
