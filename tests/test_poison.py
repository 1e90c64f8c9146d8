"""tests/poison.py itself: the byte patterns per dtype, restoration, the log, and a walk over the package that fails when an
allocation route appears that the helper does not wrap (the GPU tests would then silently stop poisoning it)."""
import ast
import glob
import math
import os
import struct

import pytest
import torch

from poison import PATTERNS, WRAPPED, poisoned, raw_equal

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep3d_aerial_amd")

# what a tensor of each dtype reads after the fill: a value, or "nan"
F32_7F = struct.unpack("<f", b"\x7f" * 4)[0]  # 3.39e38
F64_7F = struct.unpack("<d", b"\x7f" * 8)[0]  # 1.4e306
EXPECT = {
    torch.float16: {0x00: 0.0, 0xFF: "nan", 0x7F: "nan"},
    torch.bfloat16: {0x00: 0.0, 0xFF: "nan", 0x7F: F32_7F},  # 0x7F7F is finite in bf16: the fp32 pattern's top half
    torch.float32: {0x00: 0.0, 0xFF: "nan", 0x7F: F32_7F},
    torch.float64: {0x00: 0.0, 0xFF: "nan", 0x7F: F64_7F},
    torch.int32: {0x00: 0, 0xFF: -1, 0x7F: 2139062143},
    torch.int64: {0x00: 0, 0xFF: -1, 0x7F: 9187201950435737471},
    torch.uint8: {0x00: 0, 0xFF: 255, 0x7F: 127},
}


def _check(t, want):
    assert t.numel() > 0
    if want == "nan":
        assert bool(torch.isnan(t).all())
    elif t.dtype.is_floating_point:
        assert bool(torch.isfinite(t).all())
        got = t.double().reshape(-1)
        # bf16 keeps 8 bits of the fp32 pattern; every other format is exact
        tol = 2.0 ** -8 if t.dtype == torch.bfloat16 else 0.0
        assert float((got - want).abs().max()) <= tol * abs(want)
    else:
        assert bool((t == want).all())


def _h16():
    from deep3d_aerial_amd import ops

    return ops.h16_dtype()


@pytest.mark.parametrize("byte", PATTERNS)
@pytest.mark.parametrize("dtype", ["h16"] + list(EXPECT), ids=str)
def test_patterns_per_dtype(dtype, byte):
    dtype = _h16() if dtype == "h16" else dtype
    want = EXPECT[dtype][byte]
    like = torch.zeros(3, 5, dtype=torch.float32)
    with poisoned(byte) as log:
        made = [torch.empty((7, 3), dtype=dtype),
                torch.empty(2, 3, 5, dtype=dtype),
                torch.empty((), dtype=dtype),  # 0-dim
                torch.empty_like(like, dtype=dtype),  # dtype override
                torch.empty_like(like.to(dtype)),
                torch.empty_strided((4, 3), (1, 4), dtype=dtype),
                torch.empty_strided((4, 3), (8, 2), dtype=dtype),  # gaps between the elements
                like.new_empty((6,), dtype=dtype),
                like.to(dtype).new_empty(5, 2)]
    assert len(log) == len(made)
    for t in made:
        assert t.dtype == dtype
        _check(t, want)


def test_pattern_table_matches_the_documented_values():
    assert math.isclose(F32_7F, 3.39e38, rel_tol=1e-2) and math.isclose(F64_7F, 1.4e306, rel_tol=2e-2)
    assert _h16() in (torch.float16, torch.bfloat16)
    assert PATTERNS == (0x00, 0xFF, 0x7F)


def test_log_and_skips():
    with poisoned(0xFF) as log:
        assert log == []
        torch.empty((2, 3), dtype=torch.int32)
        torch.empty_like(torch.zeros(4))
        torch.empty_strided((2, 2), (2, 1))
        torch.zeros(3).new_empty((5,), dtype=torch.int64)
        z = torch.empty((0, 4))  # zero elements: nothing to fill, not logged
        torch.zeros(8)  # not an uninitialised route
    assert z.numel() == 0
    assert log[:4] == [("empty", (2, 3), torch.int32), ("empty_like", (4,), torch.float32),
                       ("empty_strided", (2, 2), torch.float32), ("new_empty", (5,), torch.int64)]
    assert all(e[1] != (0, 4) for e in log)
    assert isinstance(log, list) and log.on_device == 0      # host tensors only
    n = len(log)
    torch.empty(4)  # outside the context: not wrapped any more
    assert len(log) == n


def test_originals_restored_also_after_an_exception():
    before = [getattr(owner, name) for owner, name in WRAPPED]
    with poisoned(0x7F):
        inside = [getattr(owner, name) for owner, name in WRAPPED]
        assert all(a is not b for a, b in zip(inside, before))
    assert [getattr(owner, name) for owner, name in WRAPPED] == before
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned(0xFF):
            raise RuntimeError("boom")
    assert [getattr(owner, name) for owner, name in WRAPPED] == before
    with pytest.raises(ValueError):
        with poisoned(256):
            pass
    assert [getattr(owner, name) for owner, name in WRAPPED] == before


def test_nested_contexts_unwind_in_order():
    before = torch.empty
    with poisoned(0x00):
        with poisoned(0xFF) as inner:
            t = torch.empty(3, dtype=torch.int32)
        assert len(inner) == 1
        u = torch.empty(3, dtype=torch.int32)
    assert torch.empty is before
    assert bool((u == 0).all())
    # the inner wrapper runs last, on top of the outer one's fill
    assert bool((t == -1).all())


def test_raw_equal_counts_nans_and_signed_zeros():
    nan = torch.tensor([float("nan"), 1.0])
    assert raw_equal(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not raw_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not raw_equal(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert not raw_equal(torch.zeros(2), torch.zeros(3))
    assert raw_equal(torch.zeros(0), torch.zeros(0))
    assert raw_equal(torch.tensor([True, False]), torch.tensor([True, False]))
    assert raw_equal(torch.arange(6).reshape(2, 3).t(), torch.arange(6).reshape(2, 3).t().contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# the package's allocation routes
# ---------------------------------------------------------------------------------------------------------------------
UNWRITTEN = {"empty", "empty_like", "empty_strided", "new_empty", "resize_"}
# legacy constructors and methods that also return unwritten memory and that the helper does not wrap: none may appear
LEGACY = {"new", "FloatTensor", "DoubleTensor", "HalfTensor", "BFloat16Tensor", "IntTensor", "LongTensor", "ByteTensor",
          "ShortTensor", "CharTensor", "BoolTensor", "set_"}


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    parts.append(node.id if isinstance(node, ast.Name) else "<expr>")
    return ".".join(reversed(parts))


def _classify(path):
    """(wrapped, host, bad): calls of an unwritten-memory route in one source file, each as (line, dotted name)."""
    tree = ast.parse(open(path).read(), path)
    wrapped, host, bad = [], [], []
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            # `from torch import empty` (or an alias of torch other than `torch`) would bind the original before the helper
            # replaces it
            for a in node.names:
                if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "torch" and a.name in UNWRITTEN:
                    bad.append((node.lineno, "from torch import " + a.name))
                if isinstance(node, ast.Import) and a.name == "torch" and a.asname not in (None, "torch"):
                    bad.append((node.lineno, "import torch as " + a.asname))
            continue
        if isinstance(node, ast.Attribute) and node.attr in UNWRITTEN and not isinstance(node.ctx, ast.Load):
            bad.append((node.lineno, "assignment to " + _dotted(node)))
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Name) and (f.id in UNWRITTEN or f.id in LEGACY):
            bad.append((node.lineno, f.id))
            continue
        if not isinstance(f, ast.Attribute):
            continue
        name = _dotted(f)
        if f.attr in LEGACY and (f.attr in ("new", "set_") or name.startswith("torch.")):
            bad.append((node.lineno, name))
        if f.attr not in UNWRITTEN:
            continue
        if f.attr == "resize_":
            bad.append((node.lineno, name))  # grows a storage behind the helper's back: not allowed at all
        elif f.attr == "new_empty":
            wrapped.append((node.lineno, name))  # torch.Tensor.new_empty, whatever the tensor expression is
        elif name == "torch." + f.attr:
            wrapped.append((node.lineno, name))
        elif name == "np.empty" or name == "numpy.empty":
            host.append((node.lineno, name))  # a host numpy record, never handed to the library unwritten (see below)
        else:
            bad.append((node.lineno, name))
    # a bare reference such as `alloc = torch.empty` evaluates at call time only if it is the call's own function: any
    # other load of the attribute could keep the original alive across the patch
    calls = {id(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and node.attr in UNWRITTEN - {"resize_"} and id(node) not in calls \
                and _dotted(node).split(".")[0] in ("torch", "<expr>"):
            bad.append((node.lineno, "reference to " + _dotted(node)))
    return wrapped, host, bad


def test_every_unwritten_allocation_in_the_package_is_one_the_helper_wraps():
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) > 20
    wrapped, host, bad = {}, {}, {}
    for path in files:
        w, h, b = _classify(path)
        key = os.path.basename(path)
        if w:
            wrapped[key] = w
        if h:
            host[key] = h
        if b:
            bad[key] = b
    assert not bad, "allocation routes tests/poison.py does not wrap: %r" % bad
    # the walk does see the package's buffers (about 240 of them), so an empty result is not a pass
    total = sum(len(v) for v in wrapped.values())
    assert total >= 200, total
    for key in ("mesh.py", "ops.py", "texture.py", "fuse.py", "cloud.py", "_geom.py", "_runtime.py"):
        assert wrapped.get(key), key
    assert {name for v in wrapped.values() for _, name in v} <= {"torch.empty", "torch.empty_like", "torch.empty_strided"} | \
        {name for v in wrapped.values() for _, name in v if name.endswith(".new_empty")}
    # numpy's empty is host memory for the structured records the writers fill field by field; it never reaches a kernel.
    # Keep that list short and known: a new one is looked at before it is added here.
    assert {k: len(v) for k, v in host.items()} == {"cloud.py": 1, "cloud_compare.py": 1, "mesh.py": 1, "mesh_compare.py": 2,
                                                    "texture.py": 1}


def test_the_walk_rejects_the_routes_it_should(tmp_path):
    src = tmp_path / "m.py"
    cases = {
        "import torch\nx = torch.empty(3)\ny = x.new_empty(2)\nz = torch.empty_like(x)\n": 0,
        "import torch\nx = torch.zeros(3)\nx.resize_(9)\n": 1,
        "from torch import empty\n": 1,
        "import torch as th\nx = th.empty(3)\n": 2,
        "import torch\nalloc = torch.empty\n": 1,
        "import torch\nx = torch.zeros(1).new(4)\n": 1,
        "import torch\nx = torch.FloatTensor(4)\n": 1,
        "import torch\nx = torch.cuda.FloatTensor(4)\n": 1,
        "import torch\nx = torch.Tensor.new_empty(torch.zeros(1), (3,))\n": 0,
    }
    for text, n_bad in cases.items():
        src.write_text(text)
        assert len(_classify(str(src))[2]) == n_bad, text
