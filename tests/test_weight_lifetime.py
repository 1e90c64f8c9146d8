"""The two weight caches of _runtime.py on their own, without a GPU.

ops.derived_weight / ops._packed cache tensors made from a parameter, keyed by the parameter OBJECT (`id`, checked against a weak
reference) and validated by storage address and in-place version counter.  Captured slice loops bake the device pointers of
those tensors, so when an entry is served, remade or dropped is behaviour, not an implementation detail.  Everything here runs
on CPU tensors: _cached synchronises CUDA tensors only.
"""
import ast
import os

import pytest
import torch

from deep3d_aerial_amd import _runtime, ops

PKG = os.path.dirname(os.path.abspath(ops.__file__))
LIMIT = 4096   # a dictionary that holds more than this is cleared whole before the next entry goes in (_runtime._cached)


@pytest.fixture(autouse=True)
def _empty_caches():
    ops.clear_weight_cache()
    yield
    ops.clear_weight_cache()


class Counting:
    """fn(w) = 2 w + 1, counting its calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self, w):
        self.calls += 1
        return w * 2 + 1


def _lookups():
    """The two front ends over _cached, as (name, lookup(weight, counting fn)): derived_weight with a tag, and _cached on
    _pack_cache under _packed's key (its packing body wants a convolution weight; the cache logic under test is the same call)."""
    return [("derived", lambda w, fn: ops.derived_weight(w, "lifetime_test", fn)),
            ("packed", lambda w, fn: _runtime._cached(_runtime._pack_cache, (id(w), False), w, fn))]


@pytest.mark.parametrize("name,lookup", _lookups(), ids=[n for n, _ in _lookups()])
def test_cached_tensor_follows_the_weight(name, lookup):
    fn = Counting()
    w = torch.arange(6.0).reshape(2, 3)
    a = lookup(w, fn)
    assert fn.calls == 1 and torch.equal(a, w * 2 + 1)
    assert lookup(w, fn) is a and fn.calls == 1                      # nothing changed: a hit, the same object
    with torch.no_grad():
        w.mul_(3.0)
    b = lookup(w, fn)
    assert fn.calls == 2 and torch.equal(b, w * 2 + 1)               # in-place update: the version moved
    with torch.no_grad():
        w.copy_(torch.full((2, 3), 5.0))
    assert torch.equal(lookup(w, fn), torch.full((2, 3), 11.0)) and fn.calls == 3
    assert lookup(w, fn) is lookup(w, fn) and fn.calls == 3
    w.data = torch.full((2, 3), 7.0)                                 # a new storage: the address moved
    assert torch.equal(lookup(w, fn), torch.full((2, 3), 15.0)) and fn.calls == 4


@pytest.mark.parametrize("name,lookup", _lookups(), ids=[n for n, _ in _lookups()])
def test_data_write_hits_until_the_cache_is_cleared(name, lookup):
    """The documented hole, pinned as documented: a write through `.data` moves neither the address nor the version, so the
    stale entry is served; clear_weight_cache() is the documented step after it."""
    fn = Counting()
    w = torch.ones(4)
    lookup(w, fn)
    w.data.fill_(3.0)
    assert torch.equal(lookup(w, fn), torch.full((4,), 3.0)) and fn.calls == 1       # stale: 2 * 1 + 1
    ops.clear_weight_cache()
    assert not _runtime._derived_cache and not _runtime._pack_cache
    assert torch.equal(lookup(w, fn), torch.full((4,), 7.0)) and fn.calls == 2


@pytest.mark.parametrize("name,lookup", _lookups(), ids=[n for n, _ in _lookups()])
def test_a_new_tensor_on_a_dead_tensors_id_misses(name, lookup):
    """The caches are keyed by id(weight): a tensor object born on the address of a dead one must not be served its entry."""
    fn = Counting()
    w = torch.ones(3)
    lookup(w, fn)
    old_id = id(w)
    del w
    held, reborn = [], None
    for _ in range(4000):
        t = torch.full((3,), 2.0)
        if id(t) == old_id:
            reborn = t
            break
        held.append(t)   # (kept: the next one is a different object)
    probe = reborn if reborn is not None else held[0]
    calls = fn.calls
    assert torch.equal(lookup(probe, fn), torch.full((3,), 5.0)) and fn.calls == calls + 1
    assert lookup(probe, fn) is lookup(probe, fn) and fn.calls == calls + 1
    if reborn is None:
        pytest.fail("no new tensor object reused the dead one's id() in 4000 tries: the id-reuse lookup was not exercised")


def test_derived_of_derived_follows_the_weight():
    """ops.convtranspose2d_k3s2's wide form: `t2flip` of a weight, then `z2bf16` OF THAT RESULT -- the second entry is keyed by
    the first one's tensor, so it must be remade whenever the first is."""
    f1, f2 = Counting(), Counting()

    def chain(w):
        return ops.derived_weight(ops.derived_weight(w, "t2flip", f1), "z2bf16", f2)

    w = torch.ones(5)
    assert torch.equal(chain(w), torch.full((5,), 7.0)) and (f1.calls, f2.calls) == (1, 1)
    assert chain(w) is chain(w) and (f1.calls, f2.calls) == (1, 1)
    with torch.no_grad():
        w.mul_(2.0)
    assert torch.equal(chain(w), torch.full((5,), 11.0)) and (f1.calls, f2.calls) == (2, 2)
    w.data.fill_(0.0)
    assert torch.equal(chain(w), torch.full((5,), 11.0)) and (f1.calls, f2.calls) == (2, 2)   # the documented hole, both levels
    ops.clear_weight_cache()
    assert torch.equal(chain(w), torch.full((5,), 3.0)) and (f1.calls, f2.calls) == (3, 3)


def _fill(cache, n):
    """n distinct entries through the front end of `cache`; returns the tensors (alive: distinct ids)."""
    ws = [torch.zeros(1) for _ in range(n)]
    for t in ws:
        if cache is _runtime._derived_cache:
            ops.derived_weight(t, "lifetime_fill", lambda w: w)
        else:
            _runtime._cached(cache, (id(t), False), t, lambda w: w)
    return ws


@pytest.mark.parametrize("which", ["_derived_cache", "_pack_cache"])
def test_overflow_clears_the_whole_dictionary(which):
    """An early entry, then LIMIT + 1 distinct ones: the dictionary passed LIMIT entries and was cleared whole, so the early
    entry is made again -- and an entry of the OTHER dictionary is not."""
    cache = getattr(_runtime, which)
    other = _runtime._pack_cache if cache is _runtime._derived_cache else _runtime._derived_cache
    fn = Counting()
    early = torch.ones(2)
    first = _runtime._cached(cache, (id(early), "early"), early, fn)
    _runtime._cached(other, (id(early), "early"), early, fn)
    assert fn.calls == 2
    ws = _fill(cache, LIMIT - 1)
    assert len(cache) == LIMIT                                                # `early` and LIMIT - 1 more: nothing dropped
    assert _runtime._cached(cache, (id(early), "early"), early, fn) is first and fn.calls == 2
    ws += _fill(cache, 2)                                                     # LIMIT + 1 distinct entries behind `early`
    assert len(ws) == LIMIT + 1 and len(cache) < LIMIT
    _runtime._cached(cache, (id(early), "early"), early, fn)
    assert fn.calls == 3                                                      # the early entry went with the rest: recomputed
    _runtime._cached(other, (id(early), "early"), early, fn)
    assert fn.calls == 3                                                      # the other dictionary was not touched


# ----------------------------------------------------------------------------------------
# one packing function per tag
# ----------------------------------------------------------------------------------------
# _derived_cache is keyed (id(weight), tag) and tags are shared across call sites on purpose (conv2d_stream and conv2d_k3_pair3
# both ask for "c2s" of the same weight and get one tensor).  That is sound only while a tag means ONE function.  Tags that are
# not string constants are listed here by (file, enclosing function, tag expression); a new one fails until it is listed.
NON_CONSTANT_TAGS = {
    ("ops.py", "conv2d_k3", "'rows%d' % c0"),
    ("module.py", "_fpn_weights", "'fpn_lat' + tag"),
    ("module.py", "_fpn_weights", "'fpn_bias' + tag"),
}


def _derived_weight_calls():
    """(file, enclosing function, tag node, fn node, line) of every derived_weight(w, tag, fn) call in the package's source text."""
    found = []

    class Visitor(ast.NodeVisitor):
        def __init__(self, name):
            self.file, self.scope = name, ["<module>"]

        def visit_FunctionDef(self, node):
            self.scope.append(node.name)
            self.generic_visit(node)
            self.scope.pop()

        def visit_Call(self, node):
            f = node.func
            if (isinstance(f, ast.Name) and f.id == "derived_weight") or (isinstance(f, ast.Attribute) and f.attr == "derived_weight"):
                assert len(node.args) == 3 and not node.keywords, "%s:%d: derived_weight(weight, tag, fn), positionally" % (self.file, node.lineno)
                found.append((self.file, self.scope[-1], node.args[1], node.args[2], node.lineno))
            self.generic_visit(node)

    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as fh:
                Visitor(name).visit(ast.parse(fh.read(), name))
    return found


def test_every_tag_names_one_function():
    calls = _derived_weight_calls()
    assert len(calls) >= 50, len(calls)   # (about 60 today: the walk found the package)
    by_tag, loose = {}, set()
    for file, scope, tag, fn, line in calls:
        if isinstance(tag, ast.Constant) and isinstance(tag.value, str):
            by_tag.setdefault(tag.value, {}).setdefault(ast.dump(fn), []).append("%s:%d" % (file, line))
        else:
            loose.add((file, scope, ast.unparse(tag)))
    clashes = {t: sites for t, sites in by_tag.items() if len(sites) > 1}
    assert not clashes, "one tag, several functions: %r" % clashes
    assert loose == NON_CONSTANT_TAGS, "non-constant tags changed: %r" % sorted(loose ^ NON_CONSTANT_TAGS)
    # a built tag must not be able to spell a constant one
    for _, _, expr in NON_CONSTANT_TAGS:
        prefix = expr.split("'")[1].split("%")[0]
        assert not [t for t in by_tag if t.startswith(prefix)], (prefix, sorted(by_tag))
