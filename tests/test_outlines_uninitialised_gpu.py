"""No result of the outlines depends on what their state, offset and output buffers held before: label_outlines is run on the
129 x 67 random pattern with torch.empty and its kin pre-filled with 0x00, 0xFF and 0x7F (tests/poison.py) and must give the bits
of the plain run."""
import pytest
import torch

import objects_scene as OS
import outlines_scene as S
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu

SHAPE = (129, 67)


def _run():
    from deep3d_aerial_amd import outlines

    lab = S.labelled(OS.patterns(*SHAPE)["random_0.59"], 8)
    info = {}
    return outlines.label_outlines(torch.from_numpy(lab).cuda(), 8, info=info), info


@pytest.fixture(scope="module")
def plain():
    return _run()


@pytest.mark.parametrize("byte", PATTERNS, ids=["0x%02X" % b for b in PATTERNS])
def test_poisoned_buffers_change_nothing(plain, byte):
    want, info = plain
    with poisoned(byte) as log:
        got, got_info = _run()
    torch.cuda.synchronize()
    assert log.on_device > 0 and got_info == info and info["rings"] >= 10 and info["rounds"] >= 5
    assert all(raw_equal(got[k], want[k]) for k in ("vertices", "ring_start", "ring_object")), hex(byte)
    # the offsets, both states, the per-edge and per-ring arrays, the counters and the outputs are among the poisoned tensors
    shapes = [(shape, dtype) for _, shape, dtype in log]
    E, R, V = info["edges"], info["rings"], int(want["vertices"].shape[0])
    assert shapes.count(((E, 4), torch.int32)) == 2 and shapes.count(((E,), torch.int32)) >= 5 and shapes.count(((R,), torch.int32)) >= 3
    for expect in ((SHAPE, torch.int32), ((2,), torch.int64), ((1,), torch.int32), ((V, 2), torch.int32), ((R + 1,), torch.int32)):
        assert expect in shapes, expect
    assert any(dtype == torch.uint8 and len(shape) == 1 for shape, dtype in shapes)
