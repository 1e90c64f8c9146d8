"""CPU checks of the normal-map feature (reference mvs/mvs_cas/models/compute_normals.py:32-82, the
producer of the {view}_normal.pfm that fuse/fusion_3d_normal.py:437-443, 491-498 reads): the C ABI, its argument checks,
the CLI flags, a float64 restatement of the reference's formula against the golden data, and the file encoding."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from deep3d_aerial_amd import _lib, predict

FIXTURES = ("batch2", "holes_edge", "plane", "thin")
NORM_FLOOR = 1e-3   # pixels whose summed vector is shorter are compared for unit-vs-zero only (tests/golden/make_golden_normals.py)


def normals_f64(depth, kinv, nei):
    """compute_normals.py:32-82 evaluated in float64 with the given inv(K): P = inv(K) (x d, y d, d); the eight stencil
    differences with the reference's signs, four normalised cross products summed and normalised, a zero border of width
    nei.  Returns (normals [B,H,W,3], |summed vector| [B,H,W])."""
    depth = np.asarray(depth, np.float64)
    B, H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    P = np.einsum("bij,bhwj->bhwi", np.asarray(kinv, np.float64).reshape(B, 3, 3), np.stack([xs * depth, ys * depth, depth], -1))
    h, w = H - 2 * nei, W - 2 * nei
    at = lambda dy, dx: P[:, nei + dy:nei + dy + h, nei + dx:nei + dx + w]
    ctr = at(0, 0)
    x0, x1, y0, y1 = at(0, -nei), at(0, nei), at(-nei, 0), at(nei, 0)
    x0y0, x0y1, x1y0, x1y1 = at(-nei, -nei), at(nei, -nei), at(-nei, nei), at(nei, nei)
    unit = lambda v: v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)
    acc = (unit(np.cross(ctr - x1, y1 - ctr)) + unit(np.cross(ctr - x0, y0 - ctr)) + unit(np.cross(ctr - x0y1, x0y0 - ctr))
           + unit(np.cross(x1y0 - ctr, ctr - x1y1)))
    out, norm = np.zeros((B, H, W, 3)), np.zeros((B, H, W))
    out[:, nei:H - nei, nei:W - nei] = unit(acc)
    norm[:, nei:H - nei, nei:W - nei] = np.linalg.norm(acc, axis=-1)
    return out, norm


def chord_stats(got, want, norm):
    c = np.linalg.norm(np.asarray(got, np.float64) - want, axis=-1)[norm >= NORM_FLOOR]
    return (float(c.mean()), float(c.max())) if c.size else (0.0, 0.0)


def test_header_binding_and_library_have_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+d3d_normals_from_depth\s*\(", text)
    assert "#define D3D_ABI_VERSION 11" in text and _lib.ABI_VERSION == 11
    assert "d3d_normals_from_depth" in _lib.SIGNATURES
    _lib.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "d3d_normals_from_depth")
    assert _lib.load().d3d_version() == 11


def test_invalid_arguments_are_reported_before_any_launch():
    lib = _lib.load()
    kinv = (ctypes.c_float * 9)(*np.eye(3, dtype=np.float32).ravel().tolist())
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: every call below fails its checks first
    out = ctypes.c_void_p(1 << 30)
    assert lib.d3d_normals_from_depth(None, kinv, 1, 8, 8, 1, out, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, None, 1, 8, 8, 1, out, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, kinv, 1, 8, 8, 1, None, None, None) == -1
    assert b"no output" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, kinv, 1, 3, 8, 2, out, None, None) == -1   # H < 2 nei
    assert b"smaller than the stencil" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, kinv, 1, 8, 3, 2, out, None, None) == -1   # W < 2 nei
    assert b"smaller than the stencil" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, kinv, 1, 8, 8, 0, out, None, None) == -1   # nei < 1
    assert b"nei" in lib.d3d_last_error()
    assert lib.d3d_normals_from_depth(fake, kinv, 1, 8, 8, 1, fake, None, None) == -1  # output over the input
    assert b"alias" in lib.d3d_last_error()


def test_operator_refuses_cpu_tensors():
    from deep3d_aerial_amd import compute_normals, ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normals_from_depth(torch.ones(8, 8), np.eye(3, dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_normals.ComputeNormals().compute_normal_by_depth(torch.ones(1, 8, 8), torch.eye(3)[None], 1)


def test_cli_flags_are_accepted_and_off_by_default():
    a = predict.parse_args(["--output_folder", "o"])
    assert (a.save_normals, a.fuse_normals, a.normal_nei) == (False, False, 1)
    b = predict.parse_args(["--output_folder", "o", "--save_normals", "--fuse_normals", "--normal_nei", "2"])
    assert (b.save_normals, b.fuse_normals, b.normal_nei) == (True, True, 2)


def test_launcher_formats_the_flags_only_when_asked():
    from deep3d_aerial_amd import mvs_dl

    base = mvs_dl.MVS_Inference(96, 64, pretrain_weight="w.ckpt").argv("/d", "/o")
    assert not any("normal" in x for x in base)
    argv = mvs_dl.MVS_Inference(96, 64, pretrain_weight="w.ckpt", save_normals=True, fuse_normals=True, normal_nei=2).argv("/d", "/o")
    a = predict.parse_args(argv)
    assert (a.save_normals, a.fuse_normals, a.normal_nei) == (True, True, 2)
    s = mvs_dl.fusion_settings({"FUSION": {}})
    assert (s["estimate_normals"], s["normal_nei"]) == (False, 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference(name):
    """The restatement above against the reference's fp32 output: the chord statistics are the ones the golden generator
    recorded (the reference's own error, the yardstick of the GPU tests), and the reference gives a unit vector or zero where
    the restatement does."""
    g = load_golden("normals_" + name)
    for nei in (1, 2):
        if "ref_nei%d" % nei not in g.files:
            continue
        f64, norm = normals_f64(g["depth"], g["kinv"], nei)
        mean, mx = chord_stats(g["ref_nei%d" % nei], f64, norm)
        assert mean <= float(g["ref_chord_mean_nei%d" % nei]) * (1 + 1e-9) + 1e-15
        assert mx <= float(g["ref_chord_max_nei%d" % nei]) * (1 + 1e-9) + 1e-15
        ref = g["ref_nei%d" % nei]
        assert np.array_equal(np.linalg.norm(ref, axis=-1) > 0.5, np.linalg.norm(f64, axis=-1) > 0.5)
        H, W = ref.shape[1:3]
        border = np.ones((H, W), bool)
        border[nei:H - nei, nei:W - nei] = False
        assert not ref[:, border].any() and not f64[:, border].any()
    if name == "thin":   # H == 2 nei: all zeros
        assert not g["ref_nei2"].any()


def test_normal_pfm_decodes_back_as_the_reference_reads_it(tmp_path):
    """{view}_normal.pfm holds (n + 1) / 2 as a colour PFM; read_normal (fusion_3d_normal.py:191-195) = read_pfm * 2 - 1."""
    g = load_golden("normals_batch2")
    n = g["ref_nei1"][1]
    enc = ((n + np.float32(1.0)) * np.float32(0.5)).astype(np.float32)
    path = str(tmp_path / "v_normal.pfm")
    predict.save_pfm(path, enc)
    assert open(path, "rb").read(3) == b"PF\n"
    back, scale = predict.load_pfm(path)
    assert scale == 1.0 and back.shape == n.shape
    decoded = back * 2.0 - 1.0
    assert np.abs(decoded - n).max() <= 1.2e-7
