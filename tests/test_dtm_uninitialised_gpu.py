"""No result of the terrain filter depends on what its output, scratch and pyramid buffers held before: dsm_to_dtm is run on the
67 x 131 scene with torch.empty and its kin pre-filled with 0x00, 0xFF and 0x7F (tests/poison.py) and must give the bits of the
plain run."""
import numpy as np
import pytest
import torch

import dtm_scene as S
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu


def _run():
    from deep3d_aerial_amd import dtm
    from deep3d_aerial_amd.dsm import DsmGrid

    sc = S.scene(S.SMALL)
    H, W = sc["height"].shape
    grid = DsmGrid([0.0, W * 0.5, 0.0, H * 0.5], [0.5, 0.5], size=(W, H))
    return dtm.dsm_to_dtm(torch.from_numpy(np.array(sc["height"])).cuda(), grid, max_window=sc["max_window"])


@pytest.fixture(scope="module")
def plain():
    return _run()


@pytest.mark.parametrize("byte", PATTERNS, ids=["0x%02X" % b for b in PATTERNS])
def test_poisoned_buffers_change_nothing(plain, byte):
    with poisoned(byte) as log:
        got = _run()
    torch.cuda.synchronize()
    assert log.on_device > 0
    assert len(got) == 3 and all(raw_equal(a, b) for a, b in zip(got, plain)), hex(byte)
    # the outputs, the surfaces, the scratch of the opening and the levels of the pyramid are among the poisoned tensors
    shapes = [(shape, dtype) for _, shape, dtype in log]
    for want in (((67, 131), torch.float32), ((67, 131), torch.uint8), ((34, 66), torch.float32), ((1, 1), torch.float32)):
        assert want in shapes, want
    assert any(dtype == torch.uint8 and len(shape) == 1 and shape[0] >= 2 * 67 * 131 * 4 for shape, dtype in shapes)
