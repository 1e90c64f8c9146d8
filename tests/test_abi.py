"""CPU checks of the drop-in boundary: the C-ABI library exports every symbol the header
declares, the ctypes binding covers them all, operators refuse CPU tensors (no fallback),
and the host mirror modules are checkpoint-compatible with the reference's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from deep3d_aerial_amd import _lib


def _header_symbols():
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(d3d_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    _lib.build()
    syms = _header_symbols()
    assert len(syms) >= 19
    raw = ctypes.CDLL(_lib.SO_PATH)
    for s in syms:
        assert hasattr(raw, s), "library does not export %s" % s
    assert sorted(_lib.SIGNATURES) == syms, "ctypes binding and header disagree"
    lib = _lib.load()
    assert lib.d3d_version() == _lib.ABI_VERSION
    assert lib.d3d_last_error() is not None
    # the production build carries no experiment knob: one wrong -D in the Makefile must not ship silently
    assert lib.d3d_build_flags() == b"", lib.d3d_build_flags()
    counts = (ctypes.c_ulonglong * 4)()
    assert lib.d3d_debug_dispatch_counts(counts, 1) == 0 and lib.d3d_debug_dispatch_counts(None, 0) == -1


def test_kernel_code_table_agrees_with_the_single_kernel_hash():
    """kernel_code_table lists every kernel of the built library by mangled name; kernel_code_sha256 is its look-up by a
    unique prefix (what bench.py's counter-profile guard calls).  No absolute hash is pinned: they follow the compiler."""
    import bench

    _lib.build()
    table = _lib.kernel_code_table()
    assert all(entry is not None and entry[0] > 0 and len(entry[1]) == 64 for entry in table.values())
    headline = [name for name in table if name.startswith(bench.HEADLINE_KERNEL_PREFIX)]
    assert len(headline) == 1, headline
    assert _lib.kernel_code_sha256(bench.HEADLINE_KERNEL_PREFIX) == table[headline[0]][1]
    # a prefix that two symbols share (every instantiation of the ring kernel) identifies no kernel
    shared = "_ZN3d3d18sweep_tiled_kernelI"
    assert bench.HEADLINE_KERNEL_PREFIX.startswith(shared) and sum(name.startswith(shared) for name in table) >= 2
    assert _lib.kernel_code_sha256(shared) is None
    assert _lib.kernel_code_sha256("_ZN3d3d_no_such_kernel") is None
    # a single object file carries the same offload bundle as the library
    obj = _lib.kernel_code_table(os.path.join(_lib.CSRC, "planesweep_tiled.o"))
    assert obj and all(table[name] == entry for name, entry in obj.items())


def test_invalid_arguments_are_reported_not_thrown():
    lib = _lib.load()
    # null pointers / bad sizes must come back as D3D_ERR_INVALID_ARG before any launch
    assert lib.d3d_compose_projections(None, 3, None, None) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_softargmin_conf4(None, None, 0, 8, 4, 4, None, None, None) == -1
    assert lib.d3d_depth_range_samples(None, 0, 4, 0.0, 0, 0, None, None) == -1


def test_operators_refuse_cpu_tensors():
    from deep3d_aerial_amd import ops

    x = torch.zeros(4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.homo_warp(x, torch.zeros(12), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.variance_volume([x, x], torch.zeros(1, 12), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.softargmin_conf4(torch.zeros(4, 8, 8), torch.zeros(4))



# every public name ops.py defined before its packers and runtime helpers moved to _packing.py / _runtime.py
_OPS_PUBLIC = """AFFINE AffineDepth CONV2D_ZS_MINPIX GnStats H16_NAMES PER_PIXEL PER_PLANE avgpool_4_8 channel_last_enabled cl8_to_cl cl_to_cl8
clear_weight_cache compose_projections conv1x1_context conv1x1_upskip conv2d_k1 conv2d_k3 conv2d_k3_pair3 conv2d_k5s2_zs conv2d_s2_zs
conv2d_s2_zs_batched conv2d_same conv2d_stream conv2d_wide conv2d_zs conv3d_k3 conv3d_k3_cl conv3x3_bias_border_ conv_fold conv_k3_mfma
conv_precision convtranspose2d_k3s2 convtranspose2d_k4_zs convtranspose2d_zs convtranspose3d_k3s2 convtranspose3d_k3s2_cl
convtranspose3d_prob_cl convtranspose_k3s2_mfma depth_range_affine depth_range_host depth_range_samples derived_weight dispatch_counts
fp32_convs from_cl groupnorm_stats gru2_cell_gn gru_cell_conv_fused gru_cell_fused gru_gates gru_gates_gn gru_reset_gn gru_update
gru_update_gates_gn gru_update_gn h16_convs h16_dtype hand_over homo_warp homo_warp_double normals_from_depth normals_kinv note_depth_range
on_streams online_regress_finalize online_regress_update pair_corr_mean pair_softmax_max publish_prepared resize_bilinear
set_conv_precision side_streams slice_head_regress slice_tail_regress slice_tail_regress_same slice_tile_kernels softargmin_conf4
softargmin_conf4_var sweep_dispatch_counts to_cl uncertainty_aware_samples upsampled_conv_weight variance_volume variance_volume_cl
weighted_corr weighted_corr_cl8""".split()


def test_ops_keeps_its_names_and_shares_its_state():
    from deep3d_aerial_amd import _packing, _runtime, ops

    assert len(_OPS_PUBLIC) == 86 and [n for n in _OPS_PUBLIC if not hasattr(ops, n)] == []
    for name in ("dispatch_counts", "_gn_arenas", "_derived_cache", "_pack_cache", "_side_streams", "_depth_ranges"):
        assert getattr(ops, name) is getattr(_runtime, name), name   # one object each: imported, never copied
    assert ops._stream is _runtime._stream and ops._lib is _lib and ops.h16_dtype is _packing.h16_dtype
    assert ops._pack_z2_bf16 is _packing._pack_z2_bf16 and ops._packed_fold is _runtime._packed_fold
    # the monkeypatched constants and the operators stay defined in ops itself, next to the code that reads them
    for name in ("_CONV2D_STREAM_MIN", "CONV2D_ZS_MINPIX", "conv2d_k3", "conv3d_k3", "variance_volume_cl"):
        assert name in vars(ops) and not hasattr(_runtime, name) and not hasattr(_packing, name), name


@pytest.mark.parametrize("tag", ["model_casmvsnet_v3", "model_adamvs_v3", "model_msrednet_v3"])
def test_state_dict_is_checkpoint_compatible(tag):
    """Same keys, same order, same shapes as the reference module (recorded in the golden file)."""
    from deep3d_aerial_amd.adamvs import Infer_AdaMVSNet
    from deep3d_aerial_amd.cas_mvsnet import Infer_CascadeMVSNet
    from deep3d_aerial_amd.msrednet import Infer_CascadeREDNet

    g = load_golden(tag)
    ctor = {"casmvsnet": Infer_CascadeMVSNet, "adamvs": Infer_AdaMVSNet, "msrednet": Infer_CascadeREDNet}[tag.split("_")[1]]
    net = ctor(num_depth=int(g["num_depth"]))
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["state_shapes"]]
    # DataParallel-style 'module.' prefixed checkpoints (predict.py:100-106) load after wrapping
    wrapped = torch.nn.DataParallel(net)
    wrapped.load_state_dict({"module." + k: v for k, v in sd.items()})
