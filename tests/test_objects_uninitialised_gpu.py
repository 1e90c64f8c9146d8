"""No result of the object segmentation depends on what its output, parent, statistics and scratch buffers held before: segment is
run on the 67 x 131 scene, with and without the opening, with torch.empty and its kin pre-filled with 0x00, 0xFF and 0x7F
(tests/poison.py) and must give the bits of the plain run."""
import numpy as np
import pytest
import torch

import objects_scene as S
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu


def _run(open_):
    from deep3d_aerial_amd import objects
    from deep3d_aerial_amd.dsm import DsmGrid

    sc = S.scene(S.SMALL)
    H, W = sc["ndsm"].shape
    grid = DsmGrid(sc["border"], list(sc["unit"]), size=(W, H))
    info = {}
    label, table = objects.segment(torch.from_numpy(np.array(sc["ndsm"])).cuda(), grid, min_area=1.0, open=open_, info=info)
    return label, table, info


@pytest.fixture(scope="module", params=[0.0, 0.5], ids=["plain", "opened"])
def plain(request):
    return request.param, _run(request.param)


@pytest.mark.parametrize("byte", PATTERNS, ids=["0x%02X" % b for b in PATTERNS])
def test_poisoned_buffers_change_nothing(plain, byte):
    open_, (label, table, info) = plain
    with poisoned(byte) as log:
        got = _run(open_)
    torch.cuda.synchronize()
    assert log.on_device > 0
    assert raw_equal(got[0], label) and S.same_table(got[1], table) and table["id"].shape[0] >= 3, hex(byte)
    assert got[2]["components"] == info["components"] and got[2]["objects"] == info["objects"]
    # the parent and label rasters, the statistics, the final ids, the counters and the scratch are among the poisoned tensors
    shapes = [(shape, dtype) for _, shape, dtype in log]
    n = info["components"]
    for want in (((67, 131), torch.int32), ((n, 9), torch.int64), ((n,), torch.int32), ((2,), torch.int64)):
        assert want in shapes, want
    assert shapes.count(((67, 131), torch.int32)) >= 2
    assert any(dtype == torch.uint8 and len(shape) == 1 and shape[0] >= 67 * 131 * 4 for shape, dtype in shapes)
    if open_:
        assert ((67, 131), torch.float32) in shapes
