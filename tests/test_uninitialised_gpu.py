"""No result may depend on what an uninitialised buffer held.

The front end hands the library some 240 buffers from torch.empty / torch.empty_like.  In a fresh process the allocator mostly
serves them from new, zeroed segments, so a kernel that skips a store whose right value is 0, or reads a scratch word nobody
cleared, passes every value test.  Here every case runs three times in one process, with those buffers pre-filled with 0x00,
0xFF and 0x7F (tests/poison.py), the later runs on recycled blocks too:

  * the poisoning log is non-empty in every run, and at least one of its entries was a tensor in device memory;
  * the body of a case is the stage's own test (imported, not restated): its reference -- the numpy restatement bit for bit
    for the geometry stages, the oracle or float64 reference within that file's own constants for the operators -- holds under
    every pattern, 0xFF included;
  * every public function of the stage is spied on: the defined part of everything it returned (for a function that returns
    nothing: its tensor arguments, after the call) is bit-equal in the three runs, NaNs and signed zeros included.

The defined part of an output is what the public function's docstring says.  DEFINED below slices the outputs that have
capacity beyond a device-side count; LOOSE names the outputs that legitimately differ between runs (fp64 atomic sums: the order
of the additions; `rounds` of the two hooking loops, by function name) -- the stage's own test holds those to its reference and
its tolerance.  Scratch the package caches between calls (ops._gru2_scratch, the GroupNorm slot arenas) is dropped before every
run, so that it is allocated, and poisoned, under each pattern.

Inputs are made by the stage's test from numpy arrays (torch.from_numpy / torch.tensor / torch.zeros): none of them comes from a
route the helper wraps, except where a test builds a deliberately misaligned view inside a larger torch.empty buffer -- then the
bytes around the input are poison too, and a kernel that reads past its input shows."""
import dataclasses
import importlib
import inspect
import types

import numpy as np
import pytest
import torch

from conftest import set_switch
from poison import PATTERNS, poisoned, raw_equal

pytestmark = pytest.mark.gpu

PKG = "deep3d_aerial_amd"


# ---------------------------------------------------------------------------------------------------------------------
# the spy: what the public functions of a stage returned, reduced to the defined part
# ---------------------------------------------------------------------------------------------------------------------
# Outputs (by function name, then by key of the flattened return value) that may differ from run to run and are held to the
# reference by the stage's own test instead of bit for bit.
LOOSE = {
    "groupnorm_stats": None,          # fp64 atomic sums (csrc/gn_stats.h): the order of the additions
    "sweep_dispatch_counts": None,    # not a result: the library's running counters, which grow from run to run
}
# hooking loops: a launch may or may not see a parent another workgroup has just lowered, so how many rounds ran is no function
# of the mesh (components returns its count second: DEFINED).  Every other `rounds` is deterministic and compared.
LOOSE_KEYS = {"boundary_loops": ("rounds",), "plan_holes": ("rounds",)}


def _flatten(prefix, v, out, depth=0):
    if isinstance(v, torch.Tensor):
        out[prefix] = v.detach().cpu()
    elif isinstance(v, np.ndarray):
        out[prefix] = torch.from_numpy(np.ascontiguousarray(v)) if v.dtype.kind in "fiub" and v.dtype.names is None else v.tobytes()
    elif isinstance(v, (bool, int, float, str, bytes, type(None), np.generic)):
        out[prefix] = v
    elif depth > 6:
        return
    elif isinstance(v, dict):
        for k in v:
            _flatten("%s.%s" % (prefix, k), v[k], out, depth + 1)
    elif isinstance(v, tuple) and hasattr(v, "_fields"):
        for k in v._fields:
            _flatten("%s.%s" % (prefix, k), getattr(v, k), out, depth + 1)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _flatten("%s[%d]" % (prefix, i), x, out, depth + 1)
    elif dataclasses.is_dataclass(v) or (type(v).__module__.startswith(PKG) and hasattr(v, "__dict__")):
        for k, x in vars(v).items():
            if not k.startswith("_"):
                _flatten("%s.%s" % (prefix, k), x, out, depth + 1)
    # anything else (context managers, generators, modules, callables) carries no result


class Spy:
    """Wraps functions for the duration; records (label, {key: tensor or scalar}) per call."""

    def __init__(self, targets, defined):
        self.targets, self.defined, self.calls, self._saved = targets, defined, [], []

    def _wrap(self, name, fn):
        spy = self

        def wrapper(*args, **kwargs):
            ret = fn(*args, **kwargs)
            if name in LOOSE:
                return ret
            shown = spy.defined[name](ret, args, kwargs) if name in spy.defined else ret
            if name in LOOSE_KEYS and isinstance(shown, dict):
                shown = {k: v for k, v in shown.items() if k not in LOOSE_KEYS[name]}
            if shown is None:   # an in-place function: its tensor arguments as the call left them
                shown = [a for a in args if isinstance(a, torch.Tensor)]
            flat = {}
            _flatten(name, shown, flat)
            if flat:
                spy.calls.append(flat)
            return ret

        wrapper.__name__ = getattr(fn, "__name__", name)
        wrapper.__doc__ = getattr(fn, "__doc__", None)
        wrapper.__wrapped__ = fn
        return wrapper

    def __enter__(self):
        for owner, name in self.targets:
            fn = owner.__dict__[name] if isinstance(owner, type) else getattr(owner, name)
            self._saved.append((owner, name, fn))
            setattr(owner, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for owner, name, fn in reversed(self._saved):
            setattr(owner, name, fn)
        self._saved = []
        return False


def public_functions(module):
    """(module, name) of every public plain function a module's namespace holds: what a caller reaches as module.name."""
    return [(module, n) for n, f in sorted(vars(module).items())
            if isinstance(f, types.FunctionType) and not n.startswith("_") and f.__module__.startswith(PKG)]


def _targets(spec):
    out = []
    for s in spec:
        if isinstance(s, str) and ":" in s:            # "module:Class.method" or "module:function"
            mod, attr = s.split(":")
            owner = importlib.import_module("%s.%s" % (PKG, mod))
            parts = attr.split(".")
            for p in parts[:-1]:
                owner = getattr(owner, p)
            out.append((owner, parts[-1]))
        else:
            out += public_functions(importlib.import_module("%s.%s" % (PKG, s)))
    assert out, spec
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the stage's own test, its parameters, what to spy on
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, module, test, spy=("ops",), h16=False, force=None, conv=None, prime=None, label=None, **params):
        """prime: (name, args) of the module's cached input builder, called once before the three runs -- the inputs and the
        reference are then made outside the poisoned context, once, and shared."""
        self.module, self.test, self.spy, self.h16, self.force, self.conv, self.params = module, test, spy, h16, force, conv, params
        self.prime, self.label = prime, label

    @property
    def id(self):
        tail = [str(self.force)] * (self.force is not None) + [str(self.conv)] * (self.conv is not None) + ["h16"] * self.h16
        if self.label is not None:
            tail.append(self.label)
        else:
            tail += ["_".join(str(x) for x in v[:6]) if isinstance(v, (tuple, list)) else str(v) for v in self.params.values()]
        return "-".join([self.module.replace("test_", "").replace("_gpu", ""), self.test.replace("test_", "")] + tail)[:140]


P, RG, SV, SS = "test_parity_gpu", "test_regress_gpu", "test_sweep_views_gpu", "test_sweep_staging_gpu"
MODELS = ("cas_mvsnet:Infer_CascadeMVSNet.forward", "adamvs:Infer_AdaMVSNet.forward", "msrednet:Infer_CascadeREDNet.forward",
          "ucsnet:Infer_UCSNet.forward")


def _staging(i):
    return importlib.import_module(SS).CASES[i]


def _sweep_rows():
    R = importlib.import_module("sweep_ref")
    return R.FP32_ROWS, R.FP16_ROWS


CASES = []
# Cx, Hc, H, W of ops.gru2_cell_gn: 16 and 24 input channels on the tile kernel, 64 on the wide one; no height or width is a
# multiple of a tile, so every convolution of the cell has tile tails in the cached scratch
GRU2_SHAPES = ((8, 8, 9, 68), (16, 8, 11, 36), (32, 32, 29, 44))


def _operator_cases():
    c = CASES.append
    fp32_rows, fp16_rows = _sweep_rows()
    # --- sweeps: every kernel family forced, fp32 and fp16 storage, both layouts, the zeroed view slot, windows off the image
    for i in (1, 3):
        c(Case(SS, "test_staged_rings_repeat_the_window_kernel_and_match_the_oracle", case=_staging(i)))
    c(Case(SS, "test_staged_rings_weighted_warp_and_pair_pass"))
    c(Case(SS, "test_staged_rings_fp16_storage"))
    parity = importlib.import_module(P)
    ragged = parity.CASES[5]      # (2, 32, 37, 53, 5): not a multiple of any tile
    for forced in ("direct", "tiled", "window"):
        c(Case(P, "test_aggregation_vs_oracle", forced=forced, case=ragged))
        c(Case(P, "test_aggregation_vs_oracle", forced=forced, case=parity.CASES[8]))   # three sources on the four-view template
    for forced in ("direct", "tiled"):
        c(Case(P, "test_homo_warp_vs_oracle", forced=forced, case=ragged))
        c(Case(P, "test_homo_warp_out_of_frustum_and_nonfinite", force=forced, warp_path=forced))
    for fam in fp32_rows[0][5]:
        c(Case(SV, "test_fp32_view_counts", prime=("_fp32_inputs", (fp32_rows[0], "affine")), family=fam, row=fp32_rows[0], kind="affine"))
    c(Case(SV, "test_fp32_view_counts", prime=("_fp32_inputs", (fp32_rows[4], "pixel")), family="direct", row=fp32_rows[4], kind="pixel"))
    for fam, row in (("tiled", fp16_rows[0]), ("direct", fp16_rows[0]), ("tiled", fp16_rows[2]), ("tiled", fp16_rows[5]),
                     ("direct", fp16_rows[10])):
        c(Case(SV, "test_fp16_storage", prime=("_fp16_inputs", (row,)), family=fam, row=row))
    for fam in ("auto", "direct", "tiled", "window"):
        c(Case(SV, "test_degenerate_views_add_exact_zeros", family=fam, C=8, noise=False))
    for path_ in ("window", "tiled", "direct"):
        c(Case(P, "test_variance_volume_plane_major_is_the_same_volume", path_=path_))
    c(Case(P, "test_window_kernel_repeats_the_ring_kernel_bit_for_bit", case=parity.WINDOW_CASES[0]))
    c(Case(P, "test_window_kernel_gather_path_reads_the_channel_last_copy", C=16, V=4))
    c(Case(P, "test_variance_volume_channel_last_bf16_is_the_rounded_planar_volume", V=3, C=8, D=8, h=40, w=56, sweep=0.5))
    c(Case(P, "test_weighted_corr_cl8_is_the_rounded_planar_volume", V=5, C=16, h=70, w=100, D=8, kind="affine"))
    # --- regression, samplers, resize
    for D in (1, 9, 65):
        for with_var in (False, True):
            c(Case(RG, "test_softargmin_every_variant", D=D, with_var=with_var))
    c(Case(P, "test_softargmin_conf4"))
    c(Case(P, "test_online_regression"))
    c(Case(RG, "test_online_regression_ragged_and_resampled", H=13, W=131))
    c(Case(P, "test_pair_softmax_max"))
    for D in (5, 70):
        c(Case(RG, "test_pair_softmax_max_both_depth_modes", D=D))
    c(Case(RG, "test_uncertainty_samples_scalar_and_quad_paths", D=33))
    c(Case(RG, "test_depth_range_samples_every_form"))
    c(Case(P, "test_depth_samples_and_resize"))
    regress = importlib.import_module(RG)
    for case in (regress.RESIZE[3], regress.RESIZE[8], regress.RESIZE[9]):
        c(Case(RG, "test_resize_bilinear_grid_and_plane_loop", case=case))
    c(Case(P, "test_slice_head_regress_fused_equals_the_two_launches", transposed=True, h=70, w=100, per_pixel=False))
    c(Case(P, "test_slice_head_regress_fused_equals_the_two_launches", transposed=False, h=72, w=96, per_pixel=True))
    c(Case(P, "test_slice_tail_fused_is_the_two_launches", h=7, w=124, mode=1))
    c(Case(P, "test_slice_tail_same_resolution_is_the_two_launches", h=7, w=28, skip_after=False, bias=True, mode=1))
    c(Case(P, "test_slice_tail_same_resolution_is_the_two_launches", h=15, w=36, skip_after=True, bias=False, mode=2))
    # --- 3-D convolutions: planar and channel-last, stride 1 and 2, transposed, fp32 and h16
    for conv in ("mfma", "mfma_slice", "direct"):
        c(Case(P, "test_conv_primitives_vs_oracle", conv=conv, convpath=conv))
    c(Case(P, "test_conv3d_eight_output_channels_streaming", Ci=8, D=5, H=9, W=70))
    c(Case(P, "test_convtranspose3d_eight_output_channels_streaming", Ci=16, D=3, H=5, W=64))
    c(Case(P, "test_conv3d_single_output_channel_streaming", D=5, H=9, W=70))
    c(Case(P, "test_conv3d_zs_bf16_matrix_core_kernel", Ci=8, Co=8, D=5, H=9, W=68))
    c(Case(P, "test_convtranspose3d_zs_bf16_matrix_core_kernel", Ci=16, Co=8, D=4, H=9, W=70))
    c(Case(P, "test_convtranspose3d_zs_bf16_matrix_core_kernel", Ci=32, Co=16, D=3, H=5, W=64))
    c(Case(P, "test_conv3d_split_operand_kernel_has_fp32_accuracy", Ci=16, Co=8, D=5, H=17, W=68))
    c(Case(P, "test_convtranspose3d_split_operand_kernel_has_fp32_accuracy", Ci=16, Co=8, D=5, H=8, W=70))
    c(Case(P, "test_conv3d_stride2_split_operand_kernel_has_fp32_accuracy", Ci=8, Co=16, D=8, H=33, W=71))
    c(Case(P, "test_conv3d_stride2_channel_last_bf16", Ci=16, Co=32, D=8, H=10, W=70))
    c(Case(P, "test_convtranspose3d_channel_last_bf16", Ci=16, Co=8, D=4, H=9, W=70, fold="1"))
    c(Case(P, "test_convtranspose3d_channel_last_bf16", Ci=16, Co=8, D=4, H=9, W=70, fold="0"))
    c(Case(P, "test_convtranspose3d_channel_last_bf16", Ci=32, Co=16, D=3, H=5, W=64, fold="1"))
    c(Case(P, "test_conv3d_probability_layer_kz_folded", Ci=8, D=9, H=17, W=72, in_cl=True))
    c(Case(P, "test_conv11_prob_fused_is_the_two_layers", D=3, H=23, W=62, skip=True))
    c(Case(P, "test_conv0_takes_the_cl8_volume", h16=True, Ci=8, Co=8, D=3, H=9, W=36))
    c(Case(P, "test_volume_format_conversions"))
    # --- 2-D convolutions, the GRU cells, GroupNorm
    c(Case(P, "test_conv2d_tile_kernel_bf16_with_gru_epilogues", h16=True, Ci0=8, Ci1=8, Co=16, H=17, W=72, act=2))
    c(Case(P, "test_conv2d_tile_kernel_fp32_with_gru_epilogues", flavour="x3", Ci0=8, Ci1=8, Co=8, H=17, W=72, act=3))
    c(Case(P, "test_conv2d_wide_bf16_vs_float64_on_rounded_operands", C1=32, C2=32, Co=64, h=70, w=132, act=0))
    c(Case(P, "test_groupnorm_statistics_ride_on_the_convolution", h16=True, ci0=8, ci1=8, co=8, h=131, w=128))
    c(Case(P, "test_groupnorm_statistics_ride_on_the_convolution", h16=True, ci0=64, ci1=64, co=64, h=29, w=43))
    c(Case(P, "test_conv2d_stride2_tile_kernel_bf16", h16=True, Ci=8, Co=16, H=9, W=72, act=1))
    c(Case(P, "test_batched_stride2_convolution_is_the_per_item_launch", h16=True, B=3, Ci=16, Co=32, H=37, W=72))
    c(Case(P, "test_convtranspose2d_tile_kernel_bf16", h16=True, Ci=16, Co=8, H=9, W=36, act=1))
    c(Case(P, "test_convtranspose2d_k4_tile_kernel", Ci=32, Co=8, H=9, W=12))
    c(Case(P, "test_conv2d_5x5_stride2_tile_kernel", Ci=8, Co=16, H=131, W=256, act=0))
    c(Case(P, "test_conv2d_streaming_vector_unit_kernel", Ci=8, Co=8, H=9, W=70))
    c(Case(P, "test_conv1x1_streaming_kernel", Ci=16, Co=16, H=37, W=52, act=1, skip=True, affine=True))
    c(Case(P, "test_fpn_lateral_upsample_add", Ci=16, H=14, W=260))
    c(Case(P, "test_avgpool_4_and_8_in_one_read", C=16, H=37, W=44))
    c(Case(P, "test_pooled_context_head_fused", C=16, H=38, W=44))
    c(Case(P, "test_fpn_output_level_without_the_wide_tensor", Cl=8, Co=8, H=70, W=136, bias=True))
    c(Case(P, "test_gru_cell_fused_is_bit_identical_to_the_three_launches", C=8, stride=1, h=136, w=132))
    c(Case(P, "test_gru_cell_fused_is_bit_identical_to_the_three_launches", C=8, stride=2, h=135, w=248))
    c(Case(P, "test_gru_cell_on_streaming_kernel", Cx=16, Hc=8, H=9, W=70))
    c(Case(P, "test_trunk_conv0_pair_is_the_two_launches", hw=(264, 260)))
    c(Case(P, "test_homo_warp_double_golden_and_oracle"))
    c(Case(P, "test_stride2_and_transposed_tile_kernels_fp32", flavour="x3"))
    c(Case(P, "test_conv_gemm_channel_counts_and_epilogue", Ci=19, Co=32, mode="mfma"))
    c(Case(P, "test_conv_bf16_operands_match_rounded_oracle", Ci=24, Co=16))
    c(Case(P, "test_conv3d_channel_last_bf16", Ci=16, Co=16, D=7, H=19, W=70, in_cl=True, out_cl=True))
    c(Case(P, "test_conv3d_channel_last_bf16", Ci=8, Co=8, D=5, H=9, W=68, in_cl=False, out_cl=True))
    c(Case(P, "test_gru_cell_on_a_cl8_cost_plane_is_the_planar_cell", h16=True, C=8, h=9, w=4))
    c(Case(P, "test_groupnorm_stats_and_gates_vs_oracle"))
    for shape in GRU2_SHAPES:
        c(Case("test_uninitialised_gpu", "gru2_cell_direct", h16=True, Cx=shape[0], Hc=shape[1], H=shape[2], W=shape[3]))
    for mode in ("fp32", "h16"):
        c(Case(P, "test_gru2_split_passes_are_the_two_output_pair", mode=mode, Hc=8, h=70, w=100))
    c(Case(P, "test_gru2_split_passes_are_the_two_output_pair", mode="fp32", Hc=8, h=7, w=5))
    c(Case(P, "test_slice_gru_golden", conv="mfma", convpath="mfma"))
    c(Case(P, "test_slice_red_gru2_golden", conv="mfma", convpath="mfma"))
    c(Case(P, "test_costregnet3d_golden", conv="mfma", convpath="mfma"))
    c(Case(P, "test_pairnet_golden", conv="mfma", convpath="mfma"))
    c(Case(P, "test_ucsnet_samples_and_variance"))
    # --- the golden forwards: only the model's outputs are spied on (the captured slice loops run as they do in production)
    for tag in ("model_casmvsnet_v5", "model_adamvs_v5", "model_msrednet_v5"):
        c(Case(P, "test_model_forward_matches_reference", spy=MODELS, tag=tag))
        c(Case(P, "test_model_forward_bf16_regulariser_within_depth_budget", spy=MODELS, tag=tag))
    c(Case(P, "test_ucsnet_forward_matches_reference", spy=MODELS, tag="model_ucsnet_v5"))


def _normals_cases():
    c = CASES.append
    N = "test_normals_gpu"
    TN = importlib.import_module("test_normals")
    for name in TN.FIXTURES:
        c(Case(N, "test_kernel_against_reference_and_float64", spy=("ops", "compute_normals:ComputeNormals.compute_normal_by_depth"),
               name=name))
    c(Case(N, "test_compute_normals_forward_layout", spy=("ops", "compute_normals:ComputeNormals.forward")))
    c(Case("test_uninitialised_gpu", "normals_every_form"))


def _fusion_cases():
    c = CASES.append
    F = "test_fusion_gpu"
    spy = ("fuse", "fuse:ConsistencyChecker.check", "fuse:ViewFusion.add_source", "fuse:ViewFusion.finalize")
    c(Case(F, "test_check_bit_exact_vs_oracle", spy=spy, h=97, w=131, scale=1.25, seed=2))
    c(Case("test_uninitialised_gpu", "fusion_check_37x53", spy=spy))
    c(Case(F, "test_check_poisoned_inputs_match_oracle", spy=spy))
    c(Case(F, "test_view_fusion_matches_oracle_chain", spy=spy))
    c(Case(F, "test_fuse_block_chains_filtered_maps", spy=spy))
    for h, w in ((37, 53), (97, 131)):
        c(Case("test_uninitialised_gpu", "fusion_block_at", spy=spy, h=h, w=w))
    c(Case(F, "test_extract_points_bit_exact_vs_oracle", spy=spy, h=37, w=53, n_vis=5, skip_line=2))
    c(Case(F, "test_extract_points_bit_exact_vs_oracle", spy=spy, h=301, w=517, n_vis=11, skip_line=3))


GEOM = ("dsm", "ortho", "ortho_mesh", "mesh", "refine", "subdivide", "collapse", "flip", "texture", "cloud", "cloud_outliers",
        "cloud_compare", "mesh_compare")


def _geometry_cases():
    """Each stage's hand cases and its smallest random scene, against its *_numpy restatement (inside the stage's test)."""
    def c(module, test, label=None, prime=None, **params):
        CASES.append(Case(module, test, spy=GEOM, label=label, prime=prime, **params))

    mod = importlib.import_module
    for select, trim, mp in (("Max", 0.1, 1), ("Robust_Max", 0.1, 1), ("Robust_Max", 0.1, 4)):
        c("test_dsm_gpu", "test_exact_against_numpy", n=1000, select=select, trim=trim, min_points=mp)   # 12000 cells: most are empty
    c("test_dsm_gpu", "test_edges_outside_points_and_special_values")
    c("test_dsm_gpu", "test_moving_average_fill")
    c("test_dsm_mesh_gpu", "test_analytic_meshes_are_bit_equal_to_numpy")
    c("test_dsm_mesh_gpu", "test_random_soups_small_and_big_are_bit_equal_to_numpy", seed=0)
    c("test_dsm_mesh_gpu", "test_empty_meshes_bad_indices_and_cpu_tensors")
    c("test_ortho_gpu", "test_bit_equal_to_numpy_on_random_scenes", seed=0, tol=0.01)
    c("test_ortho_mesh_gpu", "test_the_random_scene_is_bit_equal_to_numpy", seed=0, z_down=False)
    c("test_ortho_mesh_gpu", "test_empty_meshes_and_refusals")
    c("test_mesh_gpu", "test_bit_equal_to_numpy", name="plane")
    c("test_mesh_gpu", "test_grid_not_a_multiple_of_8_and_other_settings")
    for name in sorted(mod("test_mesh_clean").HAND):
        c("test_mesh_clean_gpu", "test_hand_cases_are_bit_equal_to_numpy", name=name)
    c("test_mesh_clean_gpu", "test_random_soups_are_bit_equal_to_numpy", seed=0, n=50, m=200, hub=0)
    c("test_mesh_clean_gpu", "test_random_soups_are_bit_equal_to_numpy", seed=1, n=3000, m=2000, hub=0)
    for name in sorted(mod("test_mesh_decimate_gpu").CASES):   # (that file keeps the restatement's results: one numpy run per case)
        c("test_mesh_decimate_gpu", "test_every_pass_and_whole_runs_are_bit_equal_to_numpy", name=name)
    c("test_mesh_decimate_gpu", "test_random_soups_do_not_fault_and_are_bit_equal_to_numpy", seed=0, n=50, m=200, hub=0)
    c("test_mesh_decimate_gpu", "test_planar_grid_tetrahedron_and_adjacent_edges")
    for name in sorted(mod("test_mesh_holes").HAND):
        c("test_mesh_holes_gpu", "test_every_pass_and_the_closed_mesh_are_bit_equal_to_numpy", name=name)
    c("test_mesh_refine_gpu", "test_every_pass_is_bit_equal_to_numpy", reach=4, batch=None, reverse=False)
    c("test_mesh_refine_gpu", "test_every_pass_is_bit_equal_to_numpy", reach=1, batch=2, reverse=False)
    c("test_mesh_subdivide_gpu", "test_every_pass_is_bit_equal_to_numpy", batch=None, reverse=False)
    c("test_mesh_subdivide_gpu", "test_one_round_and_the_full_loop_equal_the_chain")
    c("test_mesh_collapse_gpu", "test_every_pass_of_a_round_is_bit_equal_to_numpy", batch=None, reverse=False)
    c("test_mesh_collapse_gpu", "test_the_loop_equals_the_chain_of_rounds_and_the_numpy_loop")
    c("test_mesh_flip_gpu", "test_every_round_of_the_chain_is_bit_equal_to_numpy")
    c("test_mesh_flip_gpu", "test_the_loop_equals_the_numpy_loop_twice_and_capped")
    c("test_texture_gpu", "test_bit_equal_to_numpy_on_random_meshes", seed=1, page_size=200, tol=0.01)
    scene = mod("test_texture_level_gpu").SCENES[0]
    c("test_texture_level_gpu", "test_graph_and_samples_are_bit_equal_to_numpy", prime=("_reference", scene), seed=scene[0], n=scene[1], n_views=scene[2])
    c("test_texture_level_gpu", "test_coverage_and_apply_are_bit_equal_given_the_same_g", prime=("_reference", scene), seed=scene[0], n=scene[1], n_views=scene[2])
    c("test_texture_level_gpu", "test_graph_of_an_empty_mesh_and_of_a_mesh_without_winners")
    scene = mod("test_texture_local_gpu").SCENES[0]
    c("test_texture_local_gpu", "test_seams_records_fold_and_band_are_bit_equal_to_numpy", prime=("_reference", scene), seed=scene[0], n=scene[1], n_views=scene[2])
    c("test_texture_local_gpu", "test_the_levelled_pages_are_bit_equal_to_numpy", prime=("_reference", scene), seed=scene[0], n=scene[1], n_views=scene[2])
    c("test_texture_smooth_gpu", "test_candidates_are_bit_equal_to_numpy_for_any_batching_and_order", batch=7, reverse=False)
    c("test_texture_smooth_gpu", "test_column_0_is_the_selections_key_and_two_halves_merge_to_the_whole")
    for rounds in (1, 9):
        c("test_texture_smooth_gpu", "test_smoothing_is_bit_equal_to_numpy_after_any_number_of_rounds", rounds=rounds)
    # (texture.face_colors allocates with torch.zeros / torch.full only: nothing of it can be poisoned, so it is no case here)
    c("test_texture_outliers_gpu", "test_the_vote_is_bit_equal_to_numpy_in_place_and_out_of_place", threshold=0.06)
    c("test_cloud_gpu", "test_no_point_one_point_and_only_dropped_points")
    for normals, colors in ((True, True), (True, False), (False, True), (False, False)):
        c("test_cloud_gpu", "test_5000_points_in_one_voxel", normals=normals, colors=colors)
    c("test_cloud_gpu", "test_the_crafted_border_tie_and_key_packing_cases")
    c("test_cloud_gpu", "test_the_crafted_filter_cases")
    c("test_cloud_outliers_gpu", "test_no_point_one_point_two_points_and_only_unkeyed_points")
    c("test_cloud_outliers_gpu", "test_5000_points_in_one_cell")
    for case in mod("test_cloud_outliers").hand_cases():
        c("test_cloud_outliers_gpu", "test_the_hand_cases", label=str(case[0]), case=case)
    for case in mod("test_cloud_compare").hand_cases():
        c("test_cloud_compare_gpu", "test_the_hand_cases", label=str(case[0]), case=case)
    c("test_cloud_compare_gpu", "test_no_query_no_target_and_only_unkeyed_points_on_either_side")
    c("test_cloud_compare_gpu", "test_query_cells_whose_window_holds_no_target_next_to_ones_that_do")
    c("test_cloud_compare_gpu", "test_the_prepared_clouds_serve_both_directions")
    for case in mod("test_mesh_compare").hand_cases():
        c("test_mesh_compare_gpu", "test_the_hand_cases", label=str(case[0]), case=case)
    c("test_mesh_compare_gpu", "test_one_face", n=17)
    c("test_mesh_compare_gpu", "test_runs_of_faces_without_samples_before_between_and_after_sampled_faces", run=255)
    c("test_mesh_compare_gpu", "test_no_face_and_only_faces_without_samples")
    c("test_mesh_compare_gpu", "test_the_face_error_is_the_scatter_restatement")


_operator_cases()
_normals_cases()
_fusion_cases()
_geometry_cases()


# ---------------------------------------------------------------------------------------------------------------------
# bodies that no existing test has at the shape the rule needs
# ---------------------------------------------------------------------------------------------------------------------
def normals_every_form(ops):
    """nei 1, 2, 3; the 16-byte and the scalar form (W % 4 != 0); encoded=True: the border band of width nei is exactly 0 in the
    normal map and exactly 0.5 in the encoded one, the two forms agree bit for bit, and the encoded map is (n + 1) / 2."""
    TG = importlib.import_module("test_normals_gpu")
    for h, w in ((20, 24), (19, 23)):
        d, K, _ = TG._plane_scene(h, w)
        d = d * (1.0 + 0.002 * np.random.default_rng(3).standard_normal(d.shape)).astype(np.float32)
        dd = torch.from_numpy(d).cuda()
        for nei in (1, 2, 3):
            n, enc = ops.normals_from_depth(dd, K, nei=nei, encoded=True)
            assert torch.equal(ops.normals_from_depth(dd, K, nei=nei), n)
            assert torch.equal(ops.normals_from_depth(dd, K, nei=nei, encoded=True, normal=False), enc)
            assert torch.equal(enc, (n + 1.0) * 0.5)
            border = torch.ones(h, w, dtype=torch.bool, device="cuda")
            border[nei:h - nei, nei:w - nei] = False
            assert int(border.sum()) > 0 and not n[border].any() and bool((enc[border] == 0.5).all())
            inner = n[nei:h - nei, nei:w - nei].reshape(-1, 3)
            assert bool(torch.isfinite(inner).all()) and float((inner.norm(dim=-1) - 1.0).abs().max()) <= 1e-5


def gru2_cell_direct(ops, Cx, Hc, H, W):
    """ops.gru2_cell_gn (ConvGRUCell2 as one library call, its three intermediates in the cached scratch set) against the cell's
    four launches made one by one from here -- the tile / wide convolution with gn=, gru_reset_gn, the convolution again,
    gru_update_gates_gn: the kernels and operands the fused call's docstring names, so bit for bit.  (ConvGRUCell2.forward itself
    would send images this small to other convolution kernels: conv2d_k3 keeps the tile kernel for CONV2D_ZS_MINPIX pixels and
    more.)"""
    from deep3d_aerial_amd import synthetic as S
    from deep3d_aerial_amd.module import ConvGRUCell2

    rng = np.random.default_rng([31, Cx, Hc, H, W])
    cell = ConvGRUCell2(Cx, Hc, 3)
    S.fill_state_dict_(cell.state_dict(), 4600 + Cx)
    cell = cell.cuda().eval()
    x = torch.from_numpy(rng.standard_normal((Cx, H, W)).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.standard_normal((Hc, H, W)).astype(np.float32)).cuda()
    rn, un, on = cell.reset_gate_norm, cell.update_gate_norm, cell.output_norm
    gc, oc = cell.gate_conv, cell.output_conv
    assert H * W < ops.CONV2D_ZS_MINPIX and not ops._gru2_scratch      # this run allocates the scratch set itself
    with torch.no_grad():
        before = ops.dispatch_counts.get("gru2_cell", 0)
        fused = ops.gru2_cell_gn(x, h, gc.weight, gc.bias, oc.weight, oc.bias, rn, un, on)
        assert fused is not None and ops.dispatch_counts.get("gru2_cell", 0) == before + 1, "the fused cell was not dispatched"
        assert len(ops._gru2_scratch) == 1
        again = ops.gru2_cell_gn(x, h, gc.weight, gc.bias, oc.weight, oc.bias, rn, un, on)   # on the scratch the first call left
        if Cx + Hc >= 64:
            conv = lambda w, b, x2, gn: ops.conv2d_wide(x, w, None, b, None, 0, x2=x2, gn=gn)
        else:
            conv = lambda w, b, x2, gn: ops.conv2d_zs(x, w, None, b, None, 0, x2=x2, skip_after_act=True, gn=gn)
        gs, go = ops.GnStats(2), ops.GnStats(1)
        f = conv(gc.weight, gc.bias, h, gs)
        assert f is not None and gs.slot is not None                    # the statistics rode on the convolution, as in the fused call
        st = gs.stats(f)
        rh = ops.gru_reset_gn(f, h, rn.weight, rn.bias, rn.eps, st[0])
        o = conv(oc.weight, oc.bias, rh, go)
        assert rh is not None and o is not None and go.slot is not None
        layers = ops.gru_update_gates_gn(o, f, h, on.weight, on.bias, un.weight, un.bias, on.eps, go.stats(o), st[1])
    print("gru2 cell %s: %d of %d values differ from the four launches, max abs %.3g"
          % ((Cx, Hc, H, W), int((fused != layers).sum()), fused.numel(), float((fused - layers).abs().max())))
    assert bool(torch.isfinite(fused).all())
    assert raw_equal(fused, again) and raw_equal(fused, layers)


def fusion_check_37x53(fuse, oracle):
    """ConsistencyChecker.check on the smallest ragged map of the fusion tests, bit for bit against the oracle."""
    from deep3d_aerial_amd import synthetic as S

    dev = importlib.import_module("test_fusion_gpu").dev
    ref, srcs = S.make_fusion_scene(37, 53, 2, seed=4)
    chk = fuse.ConsistencyChecker(1.0, 0.01, 10.0, 0.2)
    for s in srcs:
        want = oracle.fusion.consistency_check(ref["depth"], ref["normal"], ref["K"], ref["E"], s["depth"], s["normal"],
                                               s["K"], s["E"], ref["confidence"], 1.0, 0.01, 10.0, 0.2)
        got = chk.check(dev(ref["depth"]), dev(ref["normal"]), ref["K"], ref["E"], dev(s["depth"]), dev(s["normal"]),
                        s["K"], s["E"], dev(ref["confidence"]))
        assert 0 < want[0].sum() < want[0].size      # both branches of the mask
        for name, a, b in zip(("mask", "depth_reprojected", "depth_src", "xyz_world_src", "angle"), got, want):
            assert np.array_equal(a.cpu().numpy(), b), name


def fusion_block_at(fuse, oracle, h, w):
    """fuse_block against the oracle's chain (the body of the fusion file's own test) on maps of h x w."""
    importlib.import_module("test_fusion_gpu").check_fuse_block_chain(fuse, oracle, h, w)


# ---------------------------------------------------------------------------------------------------------------------
# the defined part of outputs with capacity beyond a device-side count (by public function name)
# ---------------------------------------------------------------------------------------------------------------------
def _int(t):
    return int(t.item())


DEFINED = {
    # nbr has room for 6 m entries; rows end at offset[n]
    "adjacency": lambda ret, args, kwargs: (ret[0], ret[1][:_int(ret[0][-1])], ret[2]),
    # face_index has room for 3 m entries; a refused face (repeated or out-of-range index) enters no row
    "face_incidence": lambda ret, args, kwargs: (ret[0], ret[1][:_int(ret[0][-1])]),
    # collapse.topology / flip.topology hand the two on under their keys
    "topology": lambda ret, args, kwargs: dict(ret, nbr=ret["nbr"][:_int(ret["offset"][-1])],
                                               face_index=ret["face_index"][:_int(ret["face_offset"][-1])]),
    # (vertices, faces) with room for the round's input: counts[2] vertex rows hold the mesh; the face rows past counts[1] are 0
    "faces_compact": lambda ret, args, kwargs: (ret[0][:_int(args[3][2])], ret[1]),
    "components": lambda ret, args, kwargs: ret[0],       # (labels, rounds): rounds is no function of the mesh
}


# ---------------------------------------------------------------------------------------------------------------------
# the test
# ---------------------------------------------------------------------------------------------------------------------
# module-scoped fixtures of the stages' test files, by the plain cached builder behind each: a scene and its numpy reference,
# built once (outside the poisoned context), shared by the three runs and never changed
MODULE_FIXTURES = {"candidate_scene": "candidate_scene_value", "smooth_scene": "smooth_scene_value", "crafted_rows": "crafted_rows_value"}


def _module_fixture(module, name):
    return getattr(importlib.import_module(module), MODULE_FIXTURES[name])()


def _call(case, monkeypatch, tmp_path):
    """One run of the stage's own test, with the fixtures it names."""
    from deep3d_aerial_amd import _lib, config, fuse, ops
    import oracle

    _lib.load()
    oracle.build()
    fn = getattr(importlib.import_module(case.module), case.test)
    given = {"ops": ops, "oracle": oracle, "fuse": fuse, "monkeypatch": monkeypatch, "tmp_path": tmp_path, "bf16_mode": None}
    kwargs = {}
    for name in inspect.signature(fn).parameters:
        if name in MODULE_FIXTURES:
            kwargs[name] = _module_fixture(case.module, name)
        else:
            kwargs[name] = case.params[name] if name in case.params else given[name]
    assert set(case.params) <= set(kwargs), (case.params, kwargs)
    if case.conv is not None:
        set_switch(monkeypatch, "D3D_CONV", case.conv)
    config.switches["D3D_FORCE_PATH"] = case.force or ""
    torch.manual_seed(20)      # some of the tests draw their inputs from the global generator: the same draw in every run
    if case.h16 or "bf16_mode" in kwargs:
        ops.set_conv_precision("h16")
    try:
        fn(**kwargs)
    finally:
        ops.set_conv_precision(None)
        config.switches["D3D_FORCE_PATH"] = ""


def _drop_cached_scratch():
    """The scratch the package keeps between calls: dropped, so that the next call allocates it under the run's pattern."""
    from deep3d_aerial_amd import ops

    ops._gru2_scratch.clear()
    ops._gn_arenas.clear()


def _same(a, b):
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        return raw_equal(a, b)
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_result_does_not_depend_on_what_its_buffers_held(case, monkeypatch, tmp_path):
    if case.prime is not None:
        getattr(importlib.import_module(case.module), case.prime[0])(*case.prime[1])
    for name in inspect.signature(getattr(importlib.import_module(case.module), case.test)).parameters:
        if name in MODULE_FIXTURES:
            _module_fixture(case.module, name)
    runs = []
    for byte in PATTERNS:      # in this order, in one process: the later runs also meet recycled blocks
        (tmp_path / ("%02x" % byte)).mkdir()
        _drop_cached_scratch()
        with Spy(_targets(case.spy), DEFINED) as spy:
            with monkeypatch.context() as mp:
                with poisoned(byte) as log:
                    _call(case, mp, tmp_path / ("%02x" % byte))   # asserts the stage's reference under this pattern
                    torch.cuda.synchronize()
        assert log and log.on_device > 0, "pattern %#04x: no device buffer was poisoned" % byte
        assert spy.calls, "pattern %#04x: no public function was seen" % byte
        runs.append(spy.calls)
    base = runs[0]
    for byte, other in zip(PATTERNS[1:], runs[1:]):
        assert len(other) == len(base), "pattern %#04x: %d calls, %d under 0x00" % (byte, len(other), len(base))
        diff = []
        for k, (x, y) in enumerate(zip(base, other)):
            assert list(x) == list(y), (k, list(x), list(y))
            diff += ["call %d: %s" % (k, key) for key in x if not _same(x[key], y[key])]
        assert not diff, "pattern %#04x: these outputs differ from the 0x00 run: %s" % (byte, "; ".join(diff[:20]))


def test_the_case_table_is_what_it_claims():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    for c in CASES:
        fn = getattr(importlib.import_module(c.module), c.test)
        assert set(c.params) <= set(inspect.signature(fn).parameters), c.id
