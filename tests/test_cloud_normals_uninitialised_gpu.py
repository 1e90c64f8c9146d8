"""No result of the normals or of the plane sums depends on what their output and scratch buffers held before: every stage is run
with torch.empty and its kin pre-filled with 0x00, 0xFF and 0x7F (tests/poison.py) and must give the bits of the plain run."""
import numpy as np
import pytest
import torch

import cloud_normals_scene as NS
import cloud_register_scene as S
import test_cloud as TC
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a, np.float32).reshape(-1, 3)).cuda()   # (a copy: the scene's arrays are read-only)


@pytest.fixture(scope="module")
def plain():
    """The unpoisoned results, computed once: (normals with sums of the scene, plane sums, the plane registration)."""
    from deep3d_aerial_amd import cloud_normals as CN, cloud_register as CR

    return _normals(CN), _plane_sums(CR), _register(CR)


def _normals(CN):
    return CN.estimate(_cuda(NS.scene()[0]), NS.BORDER, NS.RADIUS, return_sums=True)


def _plane_inputs():
    g = TC.unit_grid(12, 12, 12)
    rng = np.random.default_rng(4)
    moved, ref = rng.uniform(0, 12, (1000, 3)), rng.uniform(0, 12, (200, 3))
    nrm = rng.standard_normal((200, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    idx = torch.from_numpy(rng.integers(-1, 200, 1000).astype(np.int32)).cuda()
    e = torch.from_numpy(rng.integers(0, 1025, 1000).astype(np.int32)).cuda()
    return _cuda(moved), e, idx, _cuda(ref), _cuda(nrm), g


def _plane_sums(CR):
    return (CR.plane_sums(*_plane_inputs()),)


def _register(CR):
    p, q, _ = S.scene(True)
    T, log, moved = CR.register(_cuda(p[:800]), _cuda(q), S.BORDER, [1.0], max_iterations=3, metric="plane", normal_radius=1.5)
    return torch.from_numpy(T), moved


@pytest.mark.parametrize("byte", PATTERNS, ids=["0x%02X" % b for b in PATTERNS])
def test_poisoned_buffers_change_nothing(plain, byte):
    from deep3d_aerial_amd import cloud_normals as CN, cloud_register as CR

    for stage, module, want in zip((_normals, _plane_sums, _register), (CN, CR, CR), plain):
        with poisoned(byte) as log:
            got = stage(module)
        torch.cuda.synchronize()
        assert log.on_device >= 1, stage.__name__                       # the stage did allocate through the wrapped routes
        assert len(got) == len(want) and all(raw_equal(a, b) for a, b in zip(got, want)), (stage.__name__, hex(byte))
    # the normals' four outputs and their scratch, and the 87 sums, are among the poisoned tensors
    with poisoned(byte) as log:
        _normals(CN)
    shapes = [(shape, dtype) for _, shape, dtype in log]
    n = len(NS.scene()[0])
    for want in (((n, 3), torch.float32), ((n,), torch.int32), ((n, 10), torch.int64)):
        assert want in shapes, want
    assert any(dtype == torch.uint8 for _, dtype in shapes)
    with poisoned(byte) as log:
        _plane_sums(CR)
    assert ((87,), torch.int64) in [(shape, dtype) for _, shape, dtype in log]
