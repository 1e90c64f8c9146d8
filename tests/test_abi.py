"""CPU checks of the drop-in boundary: the C-ABI library exports every symbol the header
declares, the ctypes binding is derived from that header and covers them all, operators refuse CPU tensors (no fallback),
and the host mirror modules are checkpoint-compatible with the reference's."""
import ctypes
import os
import re
import subprocess

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


_SCALAR_CTYPES = {ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double,
                  ctypes.c_void_p}
_STRUCT_NAMES = ("d3d_ortho_view_t", "d3d_mesh_view_t", "d3d_mesh_grid_t")


def test_every_prototype_parses():
    """The binding is the parse of the header: every declared function, nothing but the known ctypes, the return types by census."""
    protos, structs, consts = _lib.parse_header(_lib.header_text())
    assert sorted(protos) == _header_symbols() and len(protos) >= 179
    assert sorted(structs) == sorted(_STRUCT_NAMES) and len(consts) >= 11
    for name, (args, ret) in protos.items():
        assert all(a in _SCALAR_CTYPES for a in args), name
        if name in ("d3d_last_error", "d3d_build_flags", "d3d_h16_format"):
            assert ret is ctypes.c_char_p, name
        elif name.endswith("_bytes") or name == "d3d_sweep_workspace_bytes_for":   # the sizes: size_t
            assert ret is ctypes.c_size_t, name
        elif name == "d3d_texture_local_lds_words":
            assert ret is ctypes.c_longlong, name
        else:
            assert ret is ctypes.c_int, name
        # _lib.SIGNATURES is this table in the shape its users index: argtypes, or (argtypes, restype) where not int
        assert _lib.SIGNATURES[name] == (args if ret is ctypes.c_int else (args, ret)), name
    assert protos["d3d_version"] == ([], ctypes.c_int)                                                          # (void)
    assert protos["d3d_compose_projections"][0] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert protos["d3d_dsm_scratch_bytes"][0][0] is ctypes.c_longlong and protos["d3d_texture_empty"][0][2] is ctypes.c_uint
    assert protos["d3d_online_regress_finalize"][0][3] is ctypes.c_int64 and protos["d3d_dsm_from_points"][0][2] is ctypes.c_double
    assert protos["d3d_mesh_mark"][0][0] is ctypes.c_void_p                                                     # const d3d_mesh_grid_t*
    assert [len(a) for a, _ in (protos["d3d_conv_gemm_f32"], protos["d3d_sweep_workspace_bytes_for"])] == [30, 7]


def _host_c_compiler():
    """The clang beside the hipcc that csrc/Makefile builds the library with (HIPCC, /opt/rocm/bin/hipcc by default)."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    root = os.path.dirname(os.path.dirname(hipcc))
    found = [c for c in (os.path.join(root, "llvm", "bin", "clang"), os.path.join(root, "lib", "llvm", "bin", "clang"),
                         os.path.join(os.path.dirname(hipcc), "amdclang")) if os.path.exists(c)]
    assert found, "no clang beside %s: the compiler that builds the library is needed" % hipcc
    return found[0]


def test_the_c_compiler_agrees_on_the_struct_layouts(tmp_path):
    """sizeof and every offsetof of the three records, as the C compiler lays the header's structs out, against the parsed classes."""
    from deep3d_aerial_amd import mesh, ortho

    assert ortho._ViewRecord is _lib.STRUCTS["d3d_ortho_view_t"] and mesh._ViewRecord is _lib.STRUCTS["d3d_mesh_view_t"]
    assert mesh._GridRecord is _lib.STRUCTS["d3d_mesh_grid_t"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "deep3d_planesweep.h"', 'int main(void) {']
    want = []
    for name in _STRUCT_NAMES:
        cls = _lib.STRUCTS[name]
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append("%s %d" % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
            want.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([_host_c_compiler(), "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER), "-o", str(exe), str(src)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")[:-1]
    assert got == want
    assert [ctypes.sizeof(_lib.STRUCTS[n]) for n in _STRUCT_NAMES] == [224, 192, 56]


_CRAFTED = """
#define D3D_X (-5)
#define D3D_Y 7
typedef void* d3d_stream_t;
typedef struct d3d_pair { int a, b; double m[4]; const float* p; } d3d_pair_t;
/* a comment with int d3d_not_declared(short x); inside */
const char* d3d_text(void);
size_t d3d_room(long long n, unsigned flags, const d3d_pair_t* pair, d3d_stream_t stream);
"""


def test_the_parser_reads_the_accepted_forms():
    protos, structs, consts = _lib.parse_header(_CRAFTED)
    assert consts == {"D3D_X": -5, "D3D_Y": 7}
    pair = structs["d3d_pair_t"]
    assert [f for f, _ in pair._fields_] == ["a", "b", "m", "p"] and pair.a.offset == 0 and pair.b.offset == 4
    assert (pair.m.offset, pair.m.size, pair.p.offset, ctypes.sizeof(pair)) == (8, 32, 40, 48)
    assert protos == {"d3d_text": ([], ctypes.c_char_p),
                      "d3d_room": ([ctypes.c_longlong, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_size_t)}


@pytest.mark.parametrize("text, culprits", [
    ("int d3d_narrow(int n, short x);", ("d3d_narrow", "short")),
    ("int d3d_print(const char* fmt, ...);", ("d3d_print", "...")),
    ("typedef struct d3d_named { int id; char name[8]; } d3d_named_t;", ("d3d_named_t", "char name[8]")),
    ("int d3d_first(int n) D3D_NOTHROW;\nint d3d_second(void);", ("d3d_first", "D3D_NOTHROW")),
    ("D3D_API int d3d_first(int n);", ("d3d_first", "D3D_API")),
    ("int d3d_value(d3d_pair_t pair);", ("d3d_value", "d3d_pair_t")),
    ("#define D3D_SCALE 1.5", ("D3D_SCALE", "1.5")),
    ("int d3d_matrix(const double m[16]);", ("d3d_matrix", "m[16]")),
    ("typedef struct d3d_two { float *a, *b; } d3d_two_t;", ("d3d_two_t", "float *a, *b")),
])
def test_the_parser_refuses_what_it_does_not_know(text, culprits):
    with pytest.raises(ValueError) as e:
        _lib.parse_header("typedef void* d3d_stream_t;\n" + text)
    assert all(c in str(e.value) for c in culprits), str(e.value)


def test_a_missing_header_is_reported_with_its_path(tmp_path):
    with pytest.raises(_lib.LibraryMissing, match=re.escape(str(tmp_path / "gone.h"))):
        _lib.header_text(str(tmp_path / "gone.h"))


def test_the_constants_are_read_from_the_header():
    from deep3d_aerial_amd import _runtime, fuse, mesh, ops

    c = _lib.CONSTANTS
    assert c == _lib.parse_header(_lib.header_text())[2]
    assert _lib.ABI_VERSION == c["D3D_ABI_VERSION"]
    assert (_lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_HIP) == (c["D3D_ERR_INVALID_ARG"], c["D3D_ERR_UNSUPPORTED"], c["D3D_ERR_HIP"])
    assert (_runtime.PER_PLANE, _runtime.PER_PIXEL, _runtime.AFFINE) == (c["D3D_DEPTH_PER_PLANE"], c["D3D_DEPTH_PER_PIXEL"], c["D3D_DEPTH_AFFINE"])
    assert (ops.PER_PLANE, ops.PER_PIXEL, ops.AFFINE) == (_runtime.PER_PLANE, _runtime.PER_PIXEL, _runtime.AFFINE)
    assert fuse._CAM_DOUBLES == c["D3D_FUSION_CAM_DOUBLES"] and mesh.HOLE_MAX_EDGES == c["D3D_MESH_HOLE_MAX_EDGES"]
    # read, not equal by luck: the same header with other values gives those values
    text = _lib.header_text()
    for name, value in c.items():
        other, n = re.subn(r"(#define %s) \(?-?\d+\)?" % name, r"\1 (%d)" % (value - 40), text)
        assert n == 1 and _lib.parse_header(other)[2] == dict(c, **{name: value - 40}), name
    # and no module keeps a literal beside the header's
    here = os.path.dirname(_lib.__file__)
    for module, literal in (("_lib.py", r"ABI_VERSION = \d"), ("_lib.py", r"ERR_HIP = -"), ("_runtime.py", r"AFFINE = \d"),
                            ("fuse.py", r"_CAM_DOUBLES = \d"), ("mesh.py", r"HOLE_MAX_EDGES = \d"), ("mesh.py", r"_fields_ ="),
                            ("ortho.py", r"_fields_ =")):
        assert not re.search(literal, open(os.path.join(here, module)).read()), (module, literal)


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
