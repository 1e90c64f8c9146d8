"""No result of the view selection may depend on what an uninitialised buffer held: block_references and score,
in both modes and on both paths, run under the three fill patterns of tests/poison.py in one process; everything they return is
defined (the mask is cleared by the call, score() returns only the written part of every segment), so everything must be
bit-equal, and equal to the restatement."""
import os

import numpy as np
import pytest
import torch

import view_selection_scene as VS
from deep3d_aerial_amd import sparse_model, view_selection
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu


def _flat(scores):
    return {k: getattr(scores, k) for k in ("refs", "seen", "max", "offset", "src", "score", "count")}


def test_view_selection_under_every_fill_pattern():
    model = sparse_model.load(os.path.join(VS.GOLDEN, "dense", "bin"))
    blocks, _ = view_selection.scene_blocks(model, VS.BLOCK_SIZE, VS.OVERLAP)
    blocks.append([1000.0, 1100.0, 1000.0, 1100.0, 0.0, 1.0])       # a block no point enters: its row is all zeros
    refs = model.image_ids[::-1].copy()
    cases = [(mode, lds) for mode in view_selection.MODES for lds in (None, 16)]
    runs = []
    for byte in PATTERNS:
        with poisoned(byte) as log:
            out = {"mask": view_selection.block_references(model, blocks)}
            for mode, lds in cases:
                for k, v in _flat(view_selection.score(model, refs, mode, lds_images=lds)).items():
                    out["%s/%s/%s" % (mode, lds, k)] = v
            torch.cuda.synchronize()
        assert log and log.on_device >= 1 + 6 * len(cases), (byte, log.on_device)     # the mask, and six buffers a score() call
        runs.append({k: v.cpu() for k, v in out.items()})
    for other in runs[1:]:
        assert sorted(other) == sorted(runs[0])
        for k in runs[0]:
            assert raw_equal(runs[0][k], other[k]), k
    # and what they are equal to is the rule
    assert np.array_equal(runs[0]["mask"].numpy().astype(bool), VS.references(model, blocks)) and not runs[0]["mask"][-1].any()
    for mode, lds in cases:
        get = lambda k: runs[0]["%s/%s/%s" % (mode, lds, k)].numpy()
        for i, r in enumerate(refs.tolist()):
            v = VS.view(model, r, mode)
            a, b = int(get("offset")[i]), int(get("offset")[i + 1])
            assert (int(get("seen")[i]), int(get("max")[i])) == (v["seen"], v["max"])
            assert list(zip(get("src")[a:b].tolist(), get("score")[a:b].tolist(), get("count")[a:b].tolist())) == v["sources"]
