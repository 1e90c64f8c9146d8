/*
 * deep3d_planesweep.h -- C ABI of the MI355X (gfx950) plane-sweep cost-volume engine.
 *
 * The reference (gpcv-liujin/Deep3D_Aerial) has no FFI or plugin API for this path
 * (SURVEY.md F3): its operators are Python functions and nn.Module bodies that call
 * PyTorch ATen kernels.  Each entry point below therefore replaces one such Python
 * operator (or one fused group of them) and cites it; the host-side mirror that keeps
 * the reference's names and argument meaning lives in the deep3d_aerial_amd Python package and binds
 * these symbols with ctypes (see INTEGRATION.md for the binding a maintainer would add
 * on the reference side).
 *
 * Conventions
 *   - Plain C: raw DEVICE pointers owned by the caller, explicit sizes, a HIP stream,
 *     int status.  No torch types, no exceptions across the boundary, no hidden
 *     synchronisation, no allocation: every call is stream-ordered and reentrant.  Scratch
 *     memory is the caller's: d3d_sweep_workspace_bytes() says how much a sweep can use and
 *     the sweep entry points take the buffer as (workspace, workspace_bytes).
 *   - All tensors are contiguous fp32, batch handled by the caller (the reference runs
 *     inference at batch 1, predict.py:49):
 *         features  [C,h,w]      cost volume [C,D,h,w]      maps [h,w] / [D,h,w]
 *   - Depth hypotheses are given either per plane (depth_mode = D3D_DEPTH_PER_PLANE,
 *     pointer to [D]) or per pixel (D3D_DEPTH_PER_PIXEL, pointer to [D,h,w]); both are
 *     accepted by the reference's homo_warping_float (module.py:520-521,539).
 *     D3D_DEPTH_AFFINE is the per-pixel form without the volume: the pointer is to [2,h,w] =
 *     (lo, step) maps and plane k of pixel (y,x) lies at lo[y,x] + k * step[y,x] (fp32, the
 *     product rounded, then the sum: exactly the statement of module.py:616-631, whose
 *     hypotheses are affine in the plane index).  A sweep in this mode reads two maps instead
 *     of D planes, and its results are bit-identical to the D3D_DEPTH_PER_PIXEL sweep over
 *     the volume those maps generate.  Taken by the aggregation and regression entry points
 *     (d3d_variance_volume*, d3d_weighted_corr, d3d_pair_corr_mean, d3d_softargmin_conf4*);
 *     d3d_homo_warp, d3d_homo_warp_f64coord and d3d_pair_softmax_max take modes 0 and 1 only.
 *   - proj34 is the composed homography of module.py:528-530,
 *     (src_proj @ inverse(ref_proj))[:3,:4] = [rot | trans], row-major 12 floats per
 *     source view, in DEVICE memory (d3d_compose_projections produces it).
 *   - Return value: D3D_OK, or a negative D3D_ERR_*; d3d_last_error() gives the text of
 *     the calling thread's last failure.
 *   - Sampling semantics everywhere: bilinear, per-tap zero padding,
 *     align_corners=True (module.py:548-553).  Samples whose projected
 *     coordinate is non-finite contribute 0.
 */
#ifndef DEEP3D_PLANESWEEP_H
#define DEEP3D_PLANESWEEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3D_ABI_VERSION 11

#define D3D_OK 0
#define D3D_ERR_INVALID_ARG (-1)
#define D3D_ERR_UNSUPPORTED (-2)
#define D3D_ERR_HIP (-3)

#define D3D_DEPTH_PER_PLANE 0
#define D3D_DEPTH_PER_PIXEL 1
#define D3D_DEPTH_AFFINE 2

#define D3D_MAX_VIEWS 16

/* hipStream_t without dragging HIP headers into C callers. */
typedef void* d3d_stream_t;

/* ABI version of the loaded library (== D3D_ABI_VERSION it was built with). */
int d3d_version(void);

/* Text of the calling thread's last error ("" if none). Never NULL. */
const char* d3d_last_error(void);

/*
 * module.py:528-530 -- proj = matmul(src_proj, inverse(ref_proj)); rot, trans.
 * proj44: device [V,4,4] (index 0 = reference view).  out34: device [V-1,12].
 * The 4x4 inverse and product are evaluated in double-double on the device and rounded
 * once: each entry is the fp32 value nearest to the exact composition of the fp32 inputs,
 * also for world-frame cameras whose translations of 1e5 .. 1e8 cancel.
 */
int d3d_compose_projections(const float* proj44, int n_views, float* out34, d3d_stream_t stream);

/*
 * Test hook, process-wide: 0 = the dispatcher chooses (default), 1 = direct-gather kernel, 2 = LDS-ring kernel, 3 = window kernel
 * (D3D_ERR_UNSUPPORTED where that kernel does not take the shape).  The parity suite runs every sweep case on
 * all of them.  Not for production callers.
 */
int d3d_debug_force_path(int path);

/*
 * Test hook, process-wide: out4[1] / out4[2] / out4[3] = sweep calls (homo_warp, variance, weighted, pair) served so far by the
 * direct-gather / LDS-ring / window kernel; reset != 0 clears the counters.  The model-level parity tests use it to prove that
 * the production kernels, not a fallback, produced what they compare with the reference's outputs.
 */
int d3d_debug_dispatch_counts(unsigned long long* out4, int reset);

/*
 * Compile-time experiment knobs this library was built with that differ from the production defaults, as a space-separated
 * list ("" for the production build: tests/test_abi.py asserts that).  Several -D switches of the kernels change block
 * shapes or select measured-and-dropped variants; one of them set by accident in the Makefile must not ship silently.
 */
const char* d3d_build_flags(void);

/*
 * The 16-bit operand format of this build's fast mode ("h16": every entry point named *_h16 below, BASELINE config 3): "f16"
 * (IEEE half, 11 significand bits; the default) or "bf16" (a -DD3D_H16_BF16 build).  One format per library: "h16" volumes,
 * packed weight fragments and stored activations are in it, and a caller creates them accordingly (torch.float16 /
 * torch.bfloat16).  Accumulation is fp32 either way.  Half is the default because bfloat16's 8 significand bits put the
 * regressed depth 0.9 - 1.4 stage-3 intervals from the reference's on the arg-max-sensitive model fixtures against a bar of
 * 0.25 (north_star: 1e-3 relative L1), with every rounding site of a regulariser contributing; half at the same bytes and
 * matrix-core rate stays below 0.25 (profiles/r05_h16_ablation.txt).  The variance volume, the one operand whose
 * magnitude the data decides, saturates at 65504 in the half format.  The *_bf16x3 entry points (fp32 mode: an fp32 operand as
 * the exact sum of three bfloat16 pieces) are bfloat16 in every build.
 * Replaces nothing in the reference (fp32 throughout).  ABI 9.
 */
const char* d3d_h16_format(void);

/*
 * Scratch bytes the plane-sweep entry points below (d3d_homo_warp, d3d_variance_volume[_f16],
 * d3d_weighted_corr, d3d_pair_corr_mean) can use for a problem of n_views views (reference included) of
 * [C,h,w] elements of elem_bytes (4 = fp32, 2 = fp16) swept over D planes: room for a channel-last staging
 * copy of the source maps.  0 = the shape takes none.  The buffer is the caller's (device memory, 16-byte
 * aligned, private to the call until it completes on its stream); passing NULL / fewer bytes is valid and
 * selects a slower staging form (fp32) or the direct-gather kernel (fp16).  Sweeps of at most 48 planes (the window kernel) use it
 * only when the hypotheses are a [D,h,w] VOLUME (D3D_DEPTH_PER_PIXEL): patches whose planes no window bounds then gather their
 * taps from the channel-last copy instead of the planar maps (round 4, ABI 8); (lo, step) maps and per-plane depths leave it unused.
 * Replaces nothing in the reference: torch's caching allocator plays this role there.
 */
size_t d3d_sweep_workspace_bytes(int n_views, int C, int D, int h, int w, int elem_bytes);
/* The same for a call whose depth mode is known (ABI 9): (lo, step) maps and per-plane depths never use the window kernel's
 * channel-last copy (650 MB at the last cascade stage), so their figure is the ring kernel's alone. */
size_t d3d_sweep_workspace_bytes_for(int n_views, int C, int D, int h, int w, int elem_bytes, int depth_mode);

/*
 * module.py:516-557 homo_warping_float -- warp ONE source feature map onto D planes.
 * src [C,h,w] -> out [C,D,h,w].
 */
int d3d_homo_warp(const float* src, const float* proj34, const float* depth, int depth_mode, int C, int D, int h,
                  int w, float* out, void* workspace, size_t workspace_bytes, d3d_stream_t stream);

/*
 * module.py:560-601 homo_warping_double -- the warp with an fp64 coordinate chain: proj = src_proj @ inverse(ref_proj),
 * rot @ [x,y,1], * depth, + trans, the divide and the [-1,1] normalisation in double; the grid is rounded to fp32 and
 * un-normalised / sampled in fp32 as F.grid_sample does.  (The reference function only runs when handed fp64
 * projection matrices; no model of the reference calls it.)
 * d3d_compose_projections_f64: proj44 device double [V,4,4] -> out34 device double [V-1,12].
 * d3d_homo_warp_f64coord: src [C,h,w] fp32, proj34 device double [12], depth fp32 -> out [C,D,h,w] fp32.
 */
int d3d_compose_projections_f64(const double* proj44, int n_views, double* out34, d3d_stream_t stream);
int d3d_homo_warp_f64coord(const float* src, const double* proj34, const float* depth, int depth_mode, int C, int D,
                           int h, int w, float* out, d3d_stream_t stream);

/*
 * cas_mvsnet.py:45-60 (same arithmetic ucsnet.py:119-134, msrednet.py:217-230 and,
 * with D = 1 per call, msrednet.py:400-414) -- fused warp + variance cost volume:
 *     sum = ref + SUM_i warp_i ; sq = ref^2 + SUM_i warp_i^2 ; var = sq/V - (sum/V)^2
 * feats: HOST array of n_views device pointers, feats[0] = reference [C,h,w].
 * proj34: device [V-1,12].  out: device [C,D,h,w].
 * Never materialises the warped volumes, sum or sq.
 */
int d3d_variance_volume(const float* const* feats, const float* proj34, const float* depth, int depth_mode,
                        int n_views, int C, int D, int h, int w, float* out, void* workspace, size_t workspace_bytes,
                        d3d_stream_t stream);
/* d3d_variance_volume with plane d as one contiguous block: out [D,C,h,w] (round 4, ABI 8) -- the layout the slice-recurrent
 * regularisers read (msrednet.py:400-437), as d3d_weighted_corr(plane_major = 1) is for adamvs.py:492-512.  Same values. */
int d3d_variance_volume_planes(const float* const* feats, const float* proj34, const float* depth, int depth_mode,
                               int n_views, int C, int D, int h, int w, float* out, void* workspace, size_t workspace_bytes,
                               d3d_stream_t stream);

/* d3d_variance_volume with the result as a channel-last bf16 volume [D,h,w,C] (RNE at the store; fp32 features and fp32
 * arithmetic as above): the form conv0 of the 3-D regulariser takes in bf16 mode (d3d_conv3d_k3_cl_h16, in_cl = 1), which
 * rounds its input to bf16 anyway -- so the regularised result is bit-identical to the planar fp32 route, the volume is
 * written once at half the bytes and read with 16-byte loads.  C % 8 == 0, h*w*C < 2^31, at most 6 source views;
 * D3D_ERR_UNSUPPORTED otherwise (nothing is launched; callers use d3d_variance_volume + d3d_volume_planar_to_cl_h16). */
int d3d_variance_volume_cl_h16(const float* const* feats, const float* proj34, const float* depth, int depth_mode,
                                int n_views, int C, int D, int h, int w, void* out, void* workspace, size_t workspace_bytes,
                                d3d_stream_t stream);
/* The same volume in planes of 8-channel groups, "CL8": out [D, C/8, h, w, 8] bf16 -- the 16 bytes a lane stores per voxel
 * and group are then a WHOLE cell (with C > 8 the [D,h,w,C] form above makes every store a partial 32-byte write: the
 * write traffic of a C = 16 volume was that of the planar fp32 one).  d3d_conv3d_k3_cl_h16 / d3d_conv3d_k3_c1_cl_h16 take
 * it with in_cl = 2.  For C = 8 the two layouts coincide. */
int d3d_variance_volume_cl8_h16(const float* const* feats, const float* proj34, const float* depth, int depth_mode,
                                int n_views, int C, int D, int h, int w, void* out, void* workspace, size_t workspace_bytes,
                                d3d_stream_t stream);

/* The same volume with fp16 STORAGE (BASELINE config 5): feats[i] and out are IEEE half tensors of the shapes
 * above; projections, depth and every product / sum stay fp32, the result is rounded once (RNE).  All three depth
 * modes.  The LDS-ring kernel (fp16 ring cells of 16 channels) takes C % 16 == 0 with 1 .. 6 source views, and only
 * with a workspace of d3d_sweep_workspace_bytes(..., 2) bytes: its loaders read nothing but the channel-last copy
 * they make there.  Every other call -- C not a multiple of 16 (the direct kernel then walks 8, 4 or 1 channels at a
 * time), 7 .. D3D_MAX_VIEWS - 1 source views, a null or short workspace -- runs on the direct-gather kernel: the
 * fp32 one with fp16 loads and one rounding store, so its volume is the fp32 direct kernel's rounded once. */
int d3d_variance_volume_f16(const void* const* feats, const float* proj34, const float* depth, int depth_mode,
                            int n_views, int C, int D, int h, int w, void* out, void* workspace,
                            size_t workspace_bytes, d3d_stream_t stream);

/*
 * adamvs.py:469-474 -- per-pair channel-mean correlation for the visibility net:
 *     out[d] = mean_c( ref[c] * warp_d(src)[c] )          ref, src [C,h,w] -> out [D,h,w]
 */
int d3d_pair_corr_mean(const float* ref, const float* src, const float* proj34, const float* depth, int depth_mode,
                       int C, int D, int h, int w, float* out, void* workspace, size_t workspace_bytes,
                       d3d_stream_t stream);

/*
 * adamvs.py:492-509 -- visibility-weighted correlation:
 *     sim[c,d] = SUM_i (warp_i[c,d] * ref[c]) * vw_i / (1e-5 + SUM_i vw_i)
 * weights: device [V-1,h,w] at this stage's resolution.  out [C,D,h,w] (plane_major = 0, the reference's training-time
 * layout adamvs.py:292-301) or [D,C,h,w] (plane_major = 1: the slice loop of adamvs.py:492-512 then reads plane d as one
 * contiguous [C,h,w] block -- the reference never materialises the volume at inference).
 */
int d3d_weighted_corr(const float* const* feats, const float* proj34, const float* weights, const float* depth,
                      int depth_mode, int n_views, int C, int D, int h, int w, int plane_major, float* out, void* workspace,
                      size_t workspace_bytes, d3d_stream_t stream);
/* adamvs.py:492-509 with the volume leaving as 16-bit cells in planes of 8-channel groups, out [D, C/8, h, w, 8] in the library's h16
 * format (RNE of the fp32 value d3d_weighted_corr stores; saturating at +-65504 in the half format): what the fused conv-GRU cell
 * stages with 16-byte loads (d3d_gru_cell_fused_cl8_h16).  Window kernel only -- C % 8 == 0, at most 4 source views, D <= 48: every
 * stage of the cascades -- D3D_ERR_UNSUPPORTED otherwise (the caller then takes d3d_weighted_corr).  ABI 9. */
int d3d_weighted_corr_cl8_h16(const float* const* feats, const float* proj34, const float* weights, const float* depth,
                              int depth_mode, int n_views, int C, int D, int h, int w, void* out, void* workspace,
                              size_t workspace_bytes, d3d_stream_t stream);


/*
 * cas_mvsnet.py:69-76 + module.py:605-613 -- softmax over D, soft-argmin depth and the
 * 4-plane-window confidence around trunc(SUM_k p_k k):
 * cost [D,h,w], depth ([D] or [D,h,w]) -> depth_out [h,w], conf_out [h,w].
 */
int d3d_softargmin_conf4(const float* cost, const float* depth, int depth_mode, int D, int h, int w,
                         float* depth_out, float* conf_out, d3d_stream_t stream);

/*
 * adamvs.py:514-525 (same msrednet.py:418-429) -- one plane of the online regression:
 *     p = exp(reg); max_p = max(max_p, p); sum_d += d*p; sum_p += p
 * reg [H,W].  dplane [hd,wd]: the per-pixel depth of this plane; when (hd,wd) != (H,W)
 * it is resampled bilinearly with align_corners=False (adamvs.py:519-520, the x2 case).
 * max_p, sum_d, sum_p [H,W] are updated in place (zero them before the first plane).
 */
int d3d_online_regress_update(const float* reg, const float* dplane, int hd, int wd, int H, int W, float* max_p,
                              float* sum_d, float* sum_p, d3d_stream_t stream);

/* adamvs.py:527-529 -- depth = sum_d/(sum_p+1e-10); conf = max_p/(sum_p+1e-10). */
/* The head of a slice regulariser fused with d3d_online_regress_update (bf16 mode): reg = ConvTranspose2d(8, 1, k 3, s 2, p 1,
 * output_pad 1)(up) + bias (transposed != 0: adamvs.py:417, stages 1-2; accumulators [2h,2w]) or Conv2d(8, 1, 3, pad 1)(up) + bias
 * (stage 3; accumulators [h,w]) with operands rounded to bf16 as the matrix cores round them, then the update of adamvs.py:514-525
 * with dplane [hd,wd] resampled as d3d_online_regress_update resamples it.  up [8,h,w], weight 72 floats [c][k_y][k_x] (the
 * nn.ConvTranspose2d [8,1,3,3] / nn.Conv2d [1,8,3,3] tensor, ALREADY rounded to bf16 values), bias [1]; w % 2 == 0 (transposed) /
 * w % 4 == 0, else D3D_ERR_UNSUPPORTED.  `reg` never reaches memory. */
int d3d_slice_head_regress_h16(const float* up, const float* weight, const float* bias, int transposed, const float* dplane, int hd,
                                int wd, int h, int w, float* max_p, float* sum_d, float* sum_p, d3d_stream_t stream);
/* A 3 x 3 convolution of ConvGRUCell2 (module.py:71-99: gate_conv / output_conv over cat(x, h), bias, no activation) that also
 * accumulates the GroupNorm(1, C) statistics of its output (round 4, ABI 8; csrc/gn_stats.h): gn_stats [ngroups][2] fp64 =
 * (sum, sum of squares) per channel group, ZEROED by the caller before the launch (stream order); channels >= gn_split are the second
 * group (the update half of the gate convolution), gn_split = Co means one group.  The sums are those d3d_groupnorm_stats computes
 * from the stored tensor (same operands, fp64; the order of the additions differs) -- that launch and its pass over the tensor go.
 * _zs: the tile kernel of d3d_conv2d_k3_zs_h16 for C1 + C2 = 16 | 24 | 32 | 40 (24 | 40: Co <= 16; else Co <= 32), W % 4 == 0;
 * _wide: d3d_conv2d_k3_wide_h16's shapes.  D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_conv2d_k3_zs_h16_gn(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* shift, int Co, int H,
                             int W, float* out, double* gn_stats, int gn_split, d3d_stream_t stream);
int d3d_conv2d_k3_wide_h16_gn(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* shift, int Co, int H,
                               int W, float* out, double* gn_stats, int gn_split, d3d_stream_t stream);
/* module.py:287-294 at 64 input channels (msrednet.py:348 upconv3, ABI 10): out [Co,2H,2W] = act(convT3x3_s2(in) * scale + shift)
 * (+ skip, added last) as the stride-1 convolution of the zero-stuffed input with the flipped, transposed kernel (wpacked =
 * ops._pack_z2_bf16 of it); the stuffed image exists only in the kernel's staging.  in [64,H,W]; Co = 32 | 64; 16-bit operands. */
int d3d_convtranspose2d_k3s2_wide_h16(const float* in, const void* wpacked, const float* scale, const float* shift,
                                      const float* skip, int act, int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);
/* conv0 of a feature trunk in ONE launch (round 4, ABI 7; csrc/conv2d_zs.hip, IMG3 form): out = act(scale * Conv3x3_8->Co(c) + shift)
 * with c = act0(scale0 * Conv3x3_3->8(img) + shift0) evaluated per tile from the staged image patch and never written (module.py:
 * 663-666: ConvBnReLU(3, 8) + ConvBnReLU(8, 8) at full resolution).  img [3,H,W]; w0packed [4][3][3][8] fp32 as
 * d3d_conv2d_k3_stream takes it (input channel 3 = zeros); wpacked = the split B operands of d3d_conv2d_k3_zs_bf16x3.
 * Bit-identical to d3d_conv2d_k3_stream followed by d3d_conv2d_k3_zs_bf16x3.  Co <= 16, W % 4 == 0, out 16-byte aligned;
 * D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_conv2d_k3_pair3_bf16x3(const float* img, const float* w0packed, const float* scale0, const float* shift0, int act0,
                               const void* wpacked, const float* scale, const float* shift, int act, int Co, int H, int W,
                               float* out, d3d_stream_t stream);
/* Tail of a depth slice at the stages whose head up-samples (adamvs.py:413-418, 423-425, 514-525) in ONE kernel (round 4, ABI 6;
 * csrc/regress.hip slice_tail_kernel): up = relu(ConvTranspose2d_16->8(state2) + bup + state1) stays in LDS,
 * reg = ConvTranspose2d_8->1(up) + bhead, and the online regression update of (max_p, sum_d, sum_p) [4h, 4w] at `dplane`.
 * state2 [16,h,w], state1 [8,2h,2w]; wup_packed = ops._pack_t2d_bf16, whead = the 72 head weights rounded to bf16 (fp32 values).
 * Bit-identical to d3d_convtranspose2d_k3s2_zs_h16 followed by d3d_slice_head_regress_h16(transposed = 1).  w % 4 == 0,
 * 16-byte aligned maps; D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_slice_tail_regress_h16(const float* state2, const void* wup_packed, const float* bup, const float* state1, const float* whead,
                                const float* bhead, const float* dplane, int hd, int wd, int h, int w, float* max_p, float* sum_d,
                                float* sum_p, d3d_stream_t stream);
/* The same tail with the head at `up`'s own resolution (ABI 10; adamvs.py:413-418 at the last stage, msrednet.py:361-363 + 418-437):
 * up = relu(ConvTranspose2d_16->8(state2) + bup + state1), or with skip_after_act relu(ConvTranspose2d_16->8(state2) + bup) + state1
 * (module.py:287-294 ConvTransReLU followed by the skip); reg = Conv2d(8, 1, 3, pad 1)(up) + bhead; the online regression update of
 * (max_p, sum_d, sum_p) [2h, 2w] at `dplane`.  `up` and `reg` stay in LDS.  bup may be null; whead = the [1,8,3,3] weights [c][k_y][k_x]
 * rounded to the 16-bit format (fp32 values).  Bit-identical to d3d_convtranspose2d_k3s2_zs_h16 followed by
 * d3d_slice_head_regress_h16(transposed = 0).  w % 4 == 0, 16-byte aligned maps; D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_slice_tail_regress_same_h16(const float* state2, const void* wup_packed, const float* bup, const float* state1, int skip_after_act,
                                    const float* whead, const float* bhead, const float* dplane, int hd, int wd, int h, int w,
                                    float* max_p, float* sum_d, float* sum_p, d3d_stream_t stream);
int d3d_online_regress_finalize(const float* max_p, const float* sum_d, const float* sum_p, int64_t n,
                                float* depth_out, float* conf_out, d3d_stream_t stream);

/*
 * module.py:616-650 get_depth_range_samples.
 * mode D3D_DEPTH_PER_PLANE: cur_depth is [2] = (min,max) -> out [D] = linspace.
 * mode D3D_DEPTH_PER_PIXEL: cur_depth is [h,w] -> out [D,h,w],
 *     lo = cur - D/2*interval, hi = cur + D/2*interval, out[k] = lo + k*(hi-lo)/(D-1).
 * mode D3D_DEPTH_AFFINE: cur_depth is [h,w] -> out [2,h,w] = (lo, (hi-lo)/(D-1)): the two maps the
 *     D planes of the per-pixel mode are generated from (the sweep, soft-argmin and resize entry
 *     points take them in place of the volume: cas_mvsnet.py:224-226 resamples the volume
 *     bilinearly plane by plane, which commutes with the affine form).
 */
int d3d_depth_range_samples(const float* cur_depth, int mode, int D, float interval, int h, int w, float* out,
                            d3d_stream_t stream);

/*
 * F.interpolate(mode='bilinear', align_corners=False) for a stack of n maps, as used for
 * the view weights (adamvs.py:502) and the inter-stage depth hand-off
 * (cas_mvsnet.py:211-213).  in [n,h,w] -> out [n,H,W].
 */
int d3d_resize_bilinear(const float* in, int n, int h, int w, int H, int W, float* out, d3d_stream_t stream);

/*
 * cas_mvsnet.py:224-226 -- trilinear (align_corners=False) resample of the full
 * resolution hypothesis volume [D,H,W] to the stage grid [D,h,w]; the depth axis keeps
 * its size, so this is a per-plane bilinear resize.
 * Provided as an alias of d3d_resize_bilinear with n = D.
 */

/*
 * module.py:297-304 ConvBnReLU3D / cas_mvsnet.py:84-110 -- 3x3x3 convolution, pad 1,
 * stride 1 or 2, with eval-mode BatchNorm folded to a per-channel affine
 * (scale, shift; NULL = identity), optional ReLU and optional skip tensor added AFTER
 * the activation (cas_mvsnet.py:116-118).
 * in [Ci,D,H,W]; weight [Co,Ci,3,3,3] (nn.Conv3d layout); out [Co,Do,Ho,Wo].
 */
int d3d_conv3d_k3(const float* in, const float* weight, const float* scale, const float* shift, const float* skip,
                  int relu, int Ci, int Co, int D, int H, int W, int stride, float* out, d3d_stream_t stream);

/* The same convolution for C_out = 8, stride 1 (conv0 of every CostRegNet, cas_mvsnet.py:84) on the fp32 vector units,
 * streaming the input volume through LDS plane by plane.  wpacked: the nn.Conv3d weight [8,Ci,3,3,3] re-laid out as
 * [Ci][ky][kx][kz][8] (host-side permutation, ops.conv3d_k3).  Ci % 8 == 0; returns D3D_ERR_UNSUPPORTED when
 * 7*D*H*W*4 bytes exceeds the 32-bit offsets of its staging loads. */
int d3d_conv3d_k3_co8(const float* in, const float* wpacked, const float* scale, const float* shift, const float* skip,
                      int relu, int Ci, int D, int H, int W, float* out, d3d_stream_t stream);

/* The same layer (3x3x3, stride 1, pad 1, C_out = 8; C_in = 8 | 16 | 32; W % 4 == 0) with bf16 OPERANDS on the matrix
 * cores (v_mfma_f32_16x16x32_bf16, fp32 accumulation; BASELINE config 3): tensors stay fp32 in memory, the input is
 * rounded to bf16 (RNE) while it is staged, each input plane is read once and feeds three output planes.
 * wpacked: the weight [8,Ci,3,3,3] rounded to bf16 and laid out in the instruction's B-operand order,
 * [k_z][K block of 32][lane 0..63][8 values], K = (k_y, k_x, c_in) (ops.conv3d_k3 packs it once per parameter version). */
int d3d_conv3d_k3_c8_h16(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                          int relu, int Ci, int D, int H, int W, float* out, d3d_stream_t stream);
/* The same kernel for C_out <= 16 (C_in = 8 | 16 | 32) and 32 -> 32: conv2 / conv4 of CostRegNet (cas_mvsnet.py:87,90).
 * wpacked: [k_z][K block][N tile of 16 channels][lane][8 values]. */
int d3d_conv3d_k3_zs_h16(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                          int relu, int Ci, int Co, int D, int H, int W, float* out, d3d_stream_t stream);
/* The same kernel with fp32 ACCURACY (the default precision of the regularisers): both operands as exact three-way bf16
 * splits (hi + mid + lo), six v_mfma_f32_16x16x32_bf16 products per K block accumulated in fp32 -- the 3-D form of
 * d3d_conv2d_k3_zs_bf16x3.  C_in = 8 | 16 | 32 with C_out <= 16; round 4: 32 -> 32 and 64 -> 64 (conv4 / conv6, fragments from
 * L2); W % 4 == 0.  wpacked: [hi | mid | lo] x the layout above
 * (ops._pack_c8_bf16x3). */
int d3d_conv3d_k3_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                            int relu, int Ci, int Co, int D, int H, int W, float* out, d3d_stream_t stream);
/* C_out = 1 (the probability layer) the same way: k_z folded into the columns of one tile (d3d_conv3d_k3_c1_cl_h16's form),
 * planar fp32 in [8,D,H,W] and out [D,H,W]; wpacked: [hi | mid | lo] x ops._pack_c8_kzfold_bf16. */
int d3d_conv3d_k3_c1_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                            int relu, int Ci, int D, int H, int W, float* out, d3d_stream_t stream);


/* module.py:307-314 Deconv3d (+BN+ReLU) / cas_mvsnet.py:103,118 for C_out = 8 (conv11 of CostRegNet: 16 -> 8, then the
 * skip add) on the fp32 vector units, streaming the INPUT volume through LDS: k = 3, stride 2, pad 1, output_pad 1;
 * in [Ci,D,H,W] -> out [8,2D,2H,2W]; skip (same shape as out, may be NULL) added after the activation.
 * wpacked: the nn.ConvTranspose3d weight [Ci,8,3,3,3] re-laid out as [Ci][kz][ky][kx][8].  Ci % 8 == 0. */
int d3d_convtranspose3d_k3s2_co8(const float* in, const float* wpacked, const float* scale, const float* shift,
                                 const float* skip, int relu, int Ci, int D, int H, int W, float* out,
                                 d3d_stream_t stream);

/* module.py:307-314 Deconv3d (+BN+ReLU) / cas_mvsnet.py:97-103,116-118 with bf16 OPERANDS on the matrix cores
 * (v_mfma_f32_16x16x32_bf16, fp32 accumulation; BASELINE config 3): k = 3, stride 2, pad 1, output_pad 1;
 * in [Ci,D,H,W] fp32 -> out [Co,2D,2H,2W] fp32; skip (shape of out, may be NULL) added after the activation.  Taken channel
 * pairs: 16->8, 16->16, 32->16, 64->32 (D3D_ERR_UNSUPPORTED otherwise).  The layer runs as eight dense per-parity
 * convolutions over one staged input (no multiplications by inserted zeros), each input plane read once per tile.
 * wpacked: the weight [Ci,Co,3,3,3] rounded to bf16, per output parity class in B-operand lane order
 * (ops.convtranspose3d_k3s2 packs it once per parameter version). */
int d3d_convtranspose3d_k3s2_zs_h16(const float* in, const void* wpacked, const float* scale, const float* shift,
                                     const float* skip, int relu, int Ci, int Co, int D, int H, int W, float* out,
                                     d3d_stream_t stream);
/* ... and with fp32 accuracy from three-way bf16 splits of both operands (16 -> 8 | 16: conv11 of every CostRegNet in the
 * default precision; round 4: 32 -> 16 and 64 -> 32, conv9 / conv7, the latter with its fragments read from L2); wpacked: [hi | mid | lo] x the layout above (ops._pack_t2_bf16x3). */
int d3d_convtranspose3d_k3s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift,
                                     const float* skip, int relu, int Ci, int Co, int D, int H, int W, float* out,
                                     d3d_stream_t stream);
/* Stride-2 3x3x3 convolution in fp32 accuracy on split bf16 operands (conv1 / conv3 / conv5 of a CostRegNet in fp32 mode,
 * cas_mvsnet.py:86,89,92; csrc/conv_s2x3.hip): planar fp32 in [Ci,D,H,W] -> out [Co,(D-1)/2+1,(H-1)/2+1,(W-1)/2+1];
 * wpacked = ops._pack_c8_bf16x3.  8 -> 16, 16 -> 32, 32 -> 64 with an output width that is a multiple of 4;
 * D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_conv3d_k3s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                              int relu, int Ci, int Co, int D, int H, int W, float* out, d3d_stream_t stream);

/* module.py:5-51 ConvGRUCell / adamvs.py:409-413 ConvReLU of the slice regularisers, bf16 mode: 3x3 stride-1 2-D convolution
 * over the channel concat of `in` [C1,H,W] and `in2` [C2,H,W] (may be NULL, C2 = 0) on v_mfma_f32_16x16x32_bf16, one 64 x 8
 * (32 x 8) tile of the image per step, planar fp32 tensors in HBM.  out [Co,H,W] = epilogue(conv * scale + shift):
 *   act 0 none | 1 ReLU, with `skip` [Co,H,W] (may be NULL) added before the activation or, skip_after_act, after it;
 *   act 2 GRU gates: sigmoid, channels < ep_split multiplied by h = skip [ep_split,H,W]      (-> [r*h | u]);
 *   act 3 GRU update: u*h + (1-u)*tanh(.), h = skip [Co,H,W], u = aux1 [Co,H,W].
 * C1 + C2 = 8 | 16 | 32 in groups of 8 with Co <= 32, or 48 with Co <= 48 (adamvs.py:198-238, the pair-visibility UNet);
 * W % 4 == 0; D3D_ERR_UNSUPPORTED otherwise (nothing launched).
 * wpacked: the weight [Co,C1+C2,3,3] rounded to bf16 in B-operand lane order, [K block][N tile][lane][8], K = (k_y,k_x,c_in)
 * (ops._pack_z2_bf16). */
int d3d_conv2d_k3_zs_h16(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* scale,
                          const float* shift, const float* skip, const float* aux1, int act, int ep_split,
                          int skip_after_act, int Co, int H, int W, float* out, d3d_stream_t stream);

/* The same layer in the models' default precision: exact fp32 operands on v_mfma_f32_16x16x4_f32 (weights fp32 in the same
 * [K block of 4][N tile][lane] order, ops._pack_z2_f32); arguments and shapes as d3d_conv2d_k3_zs_h16. */
int d3d_conv2d_k3_zs_f32(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* scale,
                         const float* shift, const float* skip, const float* aux1, int act, int ep_split,
                         int skip_after_act, int Co, int H, int W, float* out, d3d_stream_t stream);

/* The same layer with fp32 accuracy on the bf16 matrix cores: every fp32 operand is the exact sum of three bf16 numbers
 * (hi + mid + lo); the activations are split while a tile is staged, the weights on the host (wpacked: the three
 * d3d_conv2d_k3_zs_h16 packings of hi | mid | lo one after the other, ops._pack_z2_bf16x3), and a K block takes the six
 * products down to 2^-16 of the leading one on v_mfma_f32_16x16x32_bf16, accumulated in fp32 -- what is dropped is below
 * fp32's own rounding of a product.  Arguments and shapes as d3d_conv2d_k3_zs_f32 (C1 + C2 = 8 | 16 | 32, Co <= 32). */
int d3d_conv2d_k3_zs_bf16x3(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* scale,
                            const float* shift, const float* skip, const float* aux1, int act, int ep_split,
                            int skip_after_act, int Co, int H, int W, float* out, d3d_stream_t stream);

/* Pooled-context heads of the AdaMVS feature pyramid (adamvs.py:75-101, 116-151 of the reference:
 * out = head(cat(up(branch_4(f)), up(branch_8(f)), f)), up = bilinear resize with align_corners=False, head a 1x1 convolution
 * without bias).  d3d_avgpool2d_4_8: both AvgPool2d((4,4),4) and AvgPool2d((8,8),8) of in [C,H,W] in one read ->
 * out4 [C,H/4,W/4], out8 [C,H/8,W/8] (floor sizes; W % 4 == 0, else D3D_ERR_UNSUPPORTED).
 * d3d_conv1x1_context: out [Co,H,W] = weight [Co,Ci] . f [Ci,H,W] + resize(a [Co,Ha,Wa]) + resize(b [Co,Hb,Wb]) -- the head
 * applied to the branch outputs at THEIR resolution (a = W_a . branch_4 output, b = W_b . branch_8 output: a 1x1
 * convolution commutes with the resize), so neither the upsampled branches nor the concat reach HBM.
 * Ci == Co in 8 | 16 | 32, W % 4 == 0, 3 Wa <= W, 3 Wb <= W; D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_avgpool2d_4_8(const float* in, int C, int H, int W, float* out4, float* out8, d3d_stream_t stream);
/* module.py:677-679, 701-703 (the 1 x 1 output layers of the feature pyramids) as a streaming kernel in exact fp32 (ABI 10):
 * out [Co,H,W] = act(scale * Conv1x1(in) + shift) (+ skip, added last).  in [Ci,H,W], Ci = 8 | 16 | 32; wt = the nn.Conv2d weight
 * re-laid as [ceil(Co / 8)][Ci][8] (blocks of 8 output channels, zero-padded: ops._pack_k1); act 0 | 1 (ReLU); scale / shift / skip
 * may be null.  H * W a multiple of 4 and 16-byte aligned tensors, else D3D_ERR_UNSUPPORTED (nothing launched). */
int d3d_conv2d_k1_f32(const float* in, const float* wt, const float* scale, const float* shift, const float* skip, int act,
                      int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);

/* out [Co,H,W] -= sum over the 3x3 taps whose source pixel lies OUTSIDE the image of taps[Co,3,3]: the border correction of a
 * bias that was added to the input of a zero-padded 3x3 convolution and folded into the layer's constant (module.fpn_output:
 * the lateral bias of the last FPN level, module.py:745-747 of the reference).  In place, border pixels only. */
int d3d_conv3x3_bias_border(float* out, const float* taps, int Co, int H, int W, d3d_stream_t stream);
int d3d_conv1x1_context(const float* f, int Ci, const float* weight, const float* a, int Ha, int Wa, const float* b, int Hb,
                        int Wb, int Co, int H, int W, float* out, d3d_stream_t stream);

/* The stride-2 and the transposed (k 3, stride 2, pad 1, output_pad 1) 2-D layers of the slice regularisers on the same tile
 * scheme (adamvs.py:411 ConvReLU(8,16,3,2,1); :413-417 upconv1 16->8 with the skip before the ReLU, upconv2d 8->1): planar fp32
 * in [Ci,H,W] -> out [Co,(H-1)/2+1,(W-1)/2+1] resp. [Co,2H,2W]; act 0 | 1 (ReLU); skip (shape of out, may be NULL) added before
 * the activation or, skip_after_act, after it.  Stride 2: C_in = 8 | 16, C_out <= 32, output width % 4 == 0; transposed:
 * C_in = 8 | 16 | 32, C_out <= 16, W % 4 == 0.  wpacked: ops._pack_z2_bf16 / ops._pack_t2d_bf16 (per output parity class, as the 3-D form). */
int d3d_conv2d_k3s2_zs_h16(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                            int act, int skip_after_act, int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);
/* The same layer over `nbatch` images in ONE launch (ABI 10; msrednet.py:352-356: the encoder's stride-2 ConvReLUs depend on the cost
 * slices only, so the three of them run for every depth slice of a stage before the recurrent loop): in [nbatch][Ci,H,W],
 * out [nbatch][Co,Ho,Wo] with the given element strides between items; no skip.  Per item bit for bit d3d_conv2d_k3s2_zs_h16. */
int d3d_conv2d_k3s2_zs_h16_batched(const float* in, const void* wpacked, const float* scale, const float* shift, int act, int Ci, int Co,
                                   int H, int W, int nbatch, int64_t in_bstride, int64_t out_bstride, float* out, d3d_stream_t stream);
int d3d_convtranspose2d_k3s2_zs_h16(const float* in, const void* wpacked, const float* scale, const float* shift,
                                     const float* skip, int act, int skip_after_act, int Ci, int Co, int H, int W, float* out,
                                     d3d_stream_t stream);
/* ... and in exact fp32 (v_mfma_f32_16x16x4_f32; weights ops._pack_z2_f32 / ops._pack_t2d_f32): stride 2 takes C_in = 8 only
 * (two 65 x 17 patches of fp32 cells must fit the LDS), transposed C_in = 8 | 16 | 32. */
int d3d_conv2d_k3s2_zs_f32(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                           int act, int skip_after_act, int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);
int d3d_convtranspose2d_k3s2_zs_f32(const float* in, const void* wpacked, const float* scale, const float* shift,
                                    const float* skip, int act, int skip_after_act, int Ci, int Co, int H, int W, float* out,
                                    d3d_stream_t stream);
/* The two layers above with fp32 accuracy from three-way bf16 splits of both operands (see d3d_conv2d_k3_zs_bf16x3; wpacked:
 * the three bf16 packings of hi | mid | lo one after the other, ops._pack_z2_bf16x3 / ops._pack_t2d_bf16x3); shapes as the
 * *_zs_bf16 forms (stride 2: Ci 8 | 16; transposed: Ci 8 | 16 | 32, Co <= 16). */
int d3d_conv2d_k3s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                              int act, int skip_after_act, int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);
int d3d_convtranspose2d_k3s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift,
                                       const float* skip, int act, int skip_after_act, int Ci, int Co, int H, int W,
                                       float* out, d3d_stream_t stream);

/* ConvTranspose2d(kernel 4, stride 2, padding 1): in [Ci,H,W] -> out [Co,2H,2W], on the transposed tile kernel with split
 * operands (every output parity class has 2 x 2 taps; the patch carries a halo on both sides).  conv3x3(nearest_x2(f)) -- the
 * input side of the last FPN level, module.py:745-747 of the reference -- is this layer with summed weights
 * (ops.upsampled_conv_weight), so the upsampled tensor is never formed.  wpacked: ops._pack_t2d_k4_bf16x3 (for Co <= 8 both
 * column parities of an output row share one 16-column operand tile: ops._pack_t2d_k4fold_bf16); act 0 | 1, skip
 * [Co,2H,2W] or NULL as in the k = 3 form; Ci 8 | 16 | 32, Co <= 16, W % 4 == 0; D3D_ERR_UNSUPPORTED otherwise. */
int d3d_convtranspose2d_k4s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift,
                                       const float* skip, int act, int skip_after_act, int Ci, int Co, int H, int W,
                                       float* out, d3d_stream_t stream);

/* 3x3 stride-1 convolution over cat(in, in2) with WIDE channel counts on the bf16 matrix cores (csrc/conv2d_wide.hip; the coarse
 * conv-GRU levels of the RED-Net slice regulariser, msrednet.py:337-370 with module.py:53-99): C1 + C2 = 64 | 128 in parts of 32,
 * Co = 32 | 64 | 128; out [Co,H,W] = act(conv * scale + shift) (+ skip, added last); act 0 | 1 (ReLU).  K is walked in
 * chunks of 32 input channels (the tile kernels above keep a whole layer in LDS, which ends at 48 channels).  wpacked:
 * ops._pack_z2_bf16(weight [Co,C1+C2,3,3]).  D3D_ERR_UNSUPPORTED for other shapes. */
int d3d_conv2d_k3_wide_h16(const float* in, int C1, const float* in2, int C2, const void* wpacked, const float* scale,
                            const float* shift, const float* skip, int act, int Co, int H, int W, float* out, d3d_stream_t stream);

/* One conv-GRU cell of the slice regularisers in ONE launch (csrc/gru_fused.hip; replaces adamvs.py:409-412 conv1 + conv_gru1 resp.
 * conv2 + conv_gru2, module.py:5-51 ConvGRUCell, run as three d3d_conv2d_k3*_zs_bf16 launches before):
 *     x = relu(conv3x3_stride(cost));  r, u = sigmoid(conv3x3(cat(x, h)) + bg);  c = tanh(conv3x3(cat(x, r * h)) + bc);
 *     hout = u * h + (1 - u) * c
 * cost [CP,HI,WI], h / hout [HID,H,W] planar fp32, hout != h.  stride 1: HI, WI = H, W, CP = 8 | 16 | 32, HID = 8; stride 2:
 * H, W = (HI-1)/2+1, (WI-1)/2+1, CP = 8, HID = 16.  w1 / wg / wc: ops._pack_z2_bf16 of the three weights (bf16 matrix-core
 * operands, fp32 accumulation, the state stays fp32); bg [2 HID], bc [HID].  Bit-identical to the three-launch form.
 * W, WI multiples of 4, 16-byte aligned tensors.
 * D3D_ERR_UNSUPPORTED for other channel counts. */
int d3d_gru_cell_fused_h16(const float* cost, int CP, int HI, int WI, int stride, const float* h, int HID, int H, int W,
                            const void* w1, const void* wg, const float* bg, const void* wc, const float* bc, float* hout,
                            d3d_stream_t stream);
/* The stride-1 cell on a cost plane of channel-last 16-bit cells in 8-channel groups, cost_cl8 [CP / 8, H, W, 8] in the library's h16
 * format (one plane of d3d_weighted_corr_cl8_h16's volume): a staging task is one 16-byte load and one 16-byte LDS write, no
 * conversion, half the bytes.  Bit-identical to d3d_gru_cell_fused_h16 on the planar fp32 plane of the same values (the planar entry
 * applies the same rounding while it stages).  CP = 8 | 16 | 32, HID = 8.  ABI 9.  adamvs.py:409-410, module.py:24-51. */
int d3d_gru_cell_fused_cl8_h16(const void* cost_cl8, int CP, const float* h, int HID, int H, int W, const void* w1, const void* wg,
                               const float* bg, const void* wc, const float* bc, float* hout, d3d_stream_t stream);


/* Conv2d(kernel 5, stride 2, padding 2) -- the downsampling layers of the feature trunks (module.py:669, 675; adamvs.py:64, 70 of the reference) --
 * on the stride-2 tile kernel with split operands (fp32 accuracy): in [Ci,H,W] -> out [Co,(H-1)/2+1,(W-1)/2+1]; wpacked:
 * ops._pack_z2_bf16x3 of the weight [Co,Ci,5,5] (K = (k_y,k_x,c_in)); scale / shift / skip / act as d3d_conv2d_k3s2_zs_h16.
 * Ci 8 with Co <= 16 | Ci 16 with Co <= 32, output width % 4 == 0; D3D_ERR_UNSUPPORTED otherwise. */
int d3d_conv2d_k5s2_zs_bf16x3(const float* in, const void* wpacked, const float* scale, const float* shift, const float* skip,
                              int act, int skip_after_act, int Ci, int Co, int H, int W, float* out, d3d_stream_t stream);


/* ---- channel-last bf16 activations between the layers of a CostRegNet (bf16 mode, BASELINE config 3) ------------------
 * "CL" volume: bf16 [D][H][W][C].  The matrix-core kernels round their operands to bf16 when they stage them, so a layer
 * that hands its output on in this form loses nothing its consumer would have kept, the activation traffic halves, and a
 * staging task is one 16-byte load.  Same layers and weight packings as the *_zs_bf16 entry points above
 * (cas_mvsnet.py:84-118: conv0 planar -> CL, conv1 .. conv11 CL -> CL with CL skips, prob CL -> planar).
 *
 * d3d_conv3d_k3_cl_h16: stride 1; in_cl / out_cl select the format of `in` (also 2: CL8 [D,Ci/8,H,W,8], see
 * d3d_variance_volume_cl8_h16) and of `out` + `skip` (0: planar fp32
 *   [C,D,H,W], 1: CL).  C_in = 8 | 16 | 32, C_out <= 16 or 32 -> 32; C_out % 4 == 0 for CL output, W % 4 == 0 for planar.
 * d3d_conv3d_k3s2_cl_h16: stride 2, pad 1; CL in [D,H,W,Ci] -> CL out [(D-1)/2+1, (H-1)/2+1, (W-1)/2+1, Co];
 *   8->8, 8->16, 16->16, 16->32.
 * d3d_convtranspose3d_k3s2_cl_h16: channel_last = 1: CL in / skip / out ([2D,2H,2W,Co]); 0: the planar form above;
 *   2: CL with the x-folded weight packing (16 -> 8 only: both output-column parities in one GEMM, ops._pack_t2_fold_bf16).
 * d3d_volume_planar_to_cl_h16 / d3d_volume_cl_h16_to_planar: format conversion of a volume of n voxels, C % 8 == 0 (RNE;
 *   the way back is exact) -- for the layers that stay on the planar kernels (conv5 / conv6) and for tests.
 * D3D_ERR_UNSUPPORTED for other shapes; nothing is launched then. */
int d3d_conv3d_k3_cl_h16(const void* in, int in_cl, const void* wpacked, const float* scale, const float* shift,
                          const void* skip, int relu, int Ci, int Co, int D, int H, int W, void* out, int out_cl,
                          d3d_stream_t stream);
/* C_out = 1 (the probability layer, cas_mvsnet.py:110): in planar fp32 or CL (in_cl), out planar fp32 [D,H,W]; the three k_z
 * slices of the weight are columns 0..2 of ONE operand tile (ops._pack_c8_kzfold_bf16), a third of the matrix work of the
 * generic entry point.  C_in = 8 | 16 | 32, W % 4 == 0. */
int d3d_conv3d_k3_c1_cl_h16(const void* in, int in_cl, const void* wpacked, const float* scale, const float* shift,
                             const float* skip, int relu, int Ci, int D, int H, int W, float* out, d3d_stream_t stream);
int d3d_conv3d_k3s2_cl_h16(const void* in, const void* wpacked, const float* scale, const float* shift, const void* skip,
                            int relu, int Ci, int Co, int D, int H, int W, void* out, d3d_stream_t stream);
int d3d_convtranspose3d_k3s2_cl_h16(const void* in, const void* wpacked, const float* scale, const float* shift,
                                     const void* skip, int relu, int Ci, int Co, int D, int H, int W, void* out,
                                     int channel_last, d3d_stream_t stream);
/* conv11 + prob of a CostRegNet in one kernel (cas_mvsnet.py:103-105,118-119; csrc/conv_t2p.hip):
 *   y = skip + ReLU(scale * ConvTranspose3d_16->8(in) + shift) rounded to bf16, out = Conv3d_8->1(y) + prob_bias[0];
 * y lives in LDS only.  in CL [D,H,W,16], skip CL [2D,2H,2W,8] (or null), out planar fp32 [2D,2H,2W]; wt_folded as for
 * d3d_convtranspose3d_k3s2_cl_h16(channel_last = 2), wprob_kzfolded as for d3d_conv3d_k3_c1_cl_h16.  Bit-identical to
 * those two calls in sequence.  W even; D3D_ERR_UNSUPPORTED otherwise (nothing launched). */
int d3d_convtranspose3d_prob_cl_h16(const void* in, const void* wt_folded, const float* scale, const float* shift,
                                     const void* skip, int relu, const void* wprob_kzfolded, const float* prob_bias,
                                     int D, int H, int W, float* out, d3d_stream_t stream);
int d3d_volume_planar_to_cl_h16(const float* in, int C, size_t n, void* out, d3d_stream_t stream);
int d3d_volume_cl_h16_to_planar(const void* in, int C, size_t n, float* out, d3d_stream_t stream);


/* 3x3 stride-1 nn.Conv2d with C_out = 8 | 16 (the full- / half-resolution layers of the feature pyramids,
 * module.py:653-755, and the conv-GRU cells of the slice regularisers, module.py:5-51) on the fp32 vector units.
 * Input = cat(in0 [Ci0], in1 [Ci1]) along the channels (in1 may be NULL with Ci1 = 0; with two inputs Ci0 % 8 == 0).
 * act 0 | 1: same epilogue as d3d_conv2d_k3 (affine, ReLU, skip added after the activation); act 2 | 3: the ConvGRUCell
 * epilogues of d3d_conv_fold_f32 (2: sigmoid, channels < ep_split times h = skip; 3: u*h + (1-u)*tanh(y), u = aux1).
 * wpacked: weight [Co,Ci0+Ci1,3,3] re-laid out as [C_in rounded up to 8][ky][kx][Co], zero rows for the padding. */
int d3d_conv2d_k3_stream(const float* in0, int Ci0, const float* in1, int Ci1, const float* wpacked, const float* scale,
                         const float* shift, const float* skip, const float* aux1, int ep_split, int act, int Co, int H,
                         int W, float* out, d3d_stream_t stream);

/* module.py:736-747 (FeatureNet_mvsnet, "fpn"): out = conv1x1(in) + bias + nearest-x2 upsampling of `coarse`
 * (F.interpolate(..., scale_factor=2, mode="nearest") + self.inner(x)) without materialising the upsampled tensor.
 * in [Ci,H,W]; coarse [Co,H/2,W/2]; wpacked = weight [Co,Ci,1,1] transposed to [Ci][Co]; out [Co,H,W]; H, W even;
 * (Ci, Co) in {(8,32), (16,32)}, else D3D_ERR_UNSUPPORTED. */
int d3d_conv1x1_upskip(const float* in, int Ci, const float* wpacked, const float* bias, const float* coarse, int Co, int H,
                       int W, float* out, d3d_stream_t stream);

/*
 * cas_mvsnet.py:94-108 -- ConvTranspose3d k=3, stride 2, padding 1, output_padding 1
 * (output exactly 2x per axis) + folded BatchNorm + ReLU + skip add.
 * in [Ci,D,H,W]; weight [Ci,Co,3,3,3] (nn.ConvTranspose3d layout); out [Co,2D,2H,2W].
 */
int d3d_convtranspose3d_k3s2(const float* in, const float* weight, const float* scale, const float* shift,
                             const float* skip, int relu, int Ci, int Co, int D, int H, int W, float* out,
                             d3d_stream_t stream);

/*
 * 2D family used by the slice-recurrent regulariser (adamvs.py:403-427) and the pair
 * visibility net (adamvs.py:198-238): 3x3 conv pad 1 stride 1|2 over the channel-wise
 * concatenation of up to two inputs (torch.cat((x,h),1), module.py:30,41), with
 * per-channel affine (folded BN or bias), activation and optional skip add.
 * act: 0 none, 1 ReLU.  in1 may be NULL (then Ci1 = 0).
 * weight [Co,Ci0+Ci1,3,3].
 */
int d3d_conv2d_k3(const float* in0, int Ci0, const float* in1, int Ci1, const float* weight, const float* scale,
                  const float* shift, const float* skip, int act, int Co, int H, int W, int stride, float* out,
                  d3d_stream_t stream);

/* ConvTranspose2d k=3 stride 2 pad 1 out_pad 1 (adamvs.py:411-414). weight [Ci,Co,3,3].
 * skip (optional) is added BEFORE the activation here: adamvs.py:424,
 * relu(upconv1(x) + reg_cost1); set skip_after_act = 1 for the UNet form
 * (adamvs.py:233-235, conv4 + relu(bn(convT(x)))). */
int d3d_convtranspose2d_k3s2(const float* in, const float* weight, const float* scale, const float* shift,
                             const float* skip, int skip_after_act, int act, int Ci, int Co, int H, int W,
                             float* out, d3d_stream_t stream);

/*
 * The same convolution family on the matrix cores (v_mfma_f32_16x16x4_f32: fp32 in, fp32 accumulate,
 * numerically an fmaf chain, so parity with the fp32 reference is unchanged) as ONE implicit-GEMM
 * entry point driven by a tap list.  It serves module.py:297-304 / cas_mvsnet.py:84-121 (Conv3d,
 * ConvTranspose3d) and module.py:5-51 / adamvs.py:198-238,403-427 (Conv2d over a channel concat,
 * ConvTranspose2d); the Python host packs the weights and emits the tap lists (ops.conv_gemm).
 *   wpack  [ntaps*(Ci0+Ci1)][mpad]: packed weights, row (t*Ci + ci), mpad = 16*ceil(Co/16) (64 if 48),
 *          zero padded; value = W[co][ci][tap t] (conv) or W[ci][co][tap t] (transposed).
 *   taps_zyx [ntaps][3] (HOST, signed char): input offset of tap t; input index = g*istride + offset.
 *   The launch iterates an output grid Dg x Hg x Wg; output index = g*ostride + (oz,oy,ox) in a
 *   [Co,Do,Ho,Wo] tensor (ostride 2 = one output-parity class of a stride-2 transposed conv).
 *   scale/shift/skip/act/skip_after_act as for d3d_conv2d_k3.  2D tensors use D = Dg = Do = 1.
 */
int d3d_conv_gemm_f32(const float* in0, int Ci0, const float* in1, int Ci1, const float* wpack, int mpad,
                      const float* scale, const float* shift, const float* skip, int skip_after_act, int act,
                      int Co, int D, int H, int W, int Dg, int Hg, int Wg, int Do, int Ho, int Wo, int istride,
                      int ostride, int oz, int oy, int ox, int ntaps, const signed char* taps_zyx, float* out,
                      d3d_stream_t stream);

/*
 * z-streaming variant of the matrix-core convolution (conv_stream.hip): every input plane is staged into
 * LDS once per (x,y) tile and feeds up to three live output planes; all packed weights stay resident in
 * LDS; GEMM rows are (fold position, c_out), so narrow layers fill the 16-row MFMA tile with neighbouring
 * outputs and a stride-2 transposed convolution is ONE launch (fold = its 2x2(x2) output parities).
 * Serves the same reference modules as d3d_conv_gemm_f32; returns D3D_ERR_UNSUPPORTED when the resident
 * weights do not fit LDS (callers then use d3d_conv_gemm_f32).
 *   geom (HOST int[15]) = {Gz,Gy,Gx, cz,cy,cx, sz,sy,sx, bz,by,bx, fz,fy,fx}: column grid; per dimension
 *        input index = g*c + tap offset, output index = g*s + b + fold position (clipped to Do/Ho/Wo).
 *   M = Co*fz*fy*fx <= 64 GEMM rows, row m = ((fz_i*fy + fy_i)*fx + fx_i)*Co + co;  mpad = 16 | 32 | 64.
 *   act: 0 none, 1 ReLU, 2 = ConvGRUCell gates fused (module.py:24-38): y = sigmoid(y), and the reset-gate rows
 *        c_out < ep_split are multiplied by the state h passed in `skip` (out = [r*h | u]); 3 = ConvGRUCell state
 *        update fused (module.py:41-51): out = u*h + (1-u)*tanh(y) with h in `skip`, u in `aux1` (image kernels,
 *        <= 16 GEMM rows; otherwise D3D_ERR_UNSUPPORTED).  aux1 / ep_split are ignored for act 0 | 1.
 *   wpack [ntaps][Ci0+Ci1][mpad] (zero where a fold position does not use a tap);
 *   taps_zyx (HOST signed char[ntaps][3]) sorted by z offset, ntaps <= 128.
 */
int d3d_conv_fold_f32(const float* in0, int Ci0, const float* in1, int Ci1, const float* wpack, int mpad, int M,
                      const float* scale, const float* shift, const float* skip, int skip_after_act, int act,
                      const float* aux1, int ep_split, int Co, int D, int H, int W, int Do, int Ho, int Wo,
                      const int* geom, int ntaps, const signed char* taps_zyx, float* out, d3d_stream_t stream);

/* Same contract with bf16 MFMA operands (v_mfma_f32_16x16x16_bf16; inputs and weights rounded to nearest-even
 * bf16 as the operands are formed, fp32 accumulation, fp32 tensors in memory): the precision BASELINE.json's
 * config 3 asks for.  Depth stays within the 1e-3 relative-L1 budget of the fp32 reference (tests/test_parity_gpu.py). */
int d3d_conv_fold_h16(const float* in0, int Ci0, const float* in1, int Ci1, const float* wpack, int mpad, int M,
                       const float* scale, const float* shift, const float* skip, int skip_after_act, int act,
                       const float* aux1, int ep_split, int Co, int D, int H, int W, int Do, int Ho, int Wo,
                       const int* geom, int ntaps, const signed char* taps_zyx, float* out, d3d_stream_t stream);

/*
 * module.py:24-51 ConvGRUCell gate math, fused:
 *   phase 0: gates [2Hc,H,W] (pre-activation, bias already applied) ->
 *            r = sigmoid(gates[:Hc]); u = sigmoid(gates[Hc:]); rh = r*h; u stored.
 *   phase 1: h' = u*h + (1-u)*tanh(convc)   (in place on h allowed)
 */
int d3d_gru_gates(const float* gates, const float* h, int Hc, int64_t plane, float* rh, float* u,
                  d3d_stream_t stream);
int d3d_gru_update(const float* u, const float* h, const float* convc, int64_t n, float* h_out,
                   d3d_stream_t stream);

/*
 * module.py:53-99 ConvGRUCell2 (msrednet.py:337-371): like ConvGRUCell, but every convolution output passes
 * nn.GroupNorm(1, C) (one group: statistics over all C*H*W elements; per-channel gamma/beta) first.
 *   d3d_groupnorm_stats: x holds ngroups consecutive segments of n elements; stats[2g] = sum, stats[2g+1] = sum of
 *     squares of segment g (device doubles; zeroed by the call, stream-ordered).  The r and u halves of the gate
 *     tensor are two segments of one call.
 *   d3d_gru_gates_gn:  r = sigmoid(gn_r(gates[:Hc])); u = sigmoid(gn_u(gates[Hc:])); rh = r*h.
 *   d3d_gru_update_gn: h' = u*h + (1-u)*tanh(gn_o(o)).
 * fast (ABI 9): 0 = torch's own expressions (IEEE division, tanhf: the fp32 mode), 1 = the one-exp-one-rcp forms the h16 kernels
 * use (about 2e-7 from the exact value; these launches are ~15 us each, 2816 of them per RED-Net view).
 */
int d3d_groupnorm_stats(const float* x, int64_t n, int ngroups, double* stats, d3d_stream_t stream);
int d3d_gru_gates_gn(const float* gates, const double* stats_r, const double* stats_u, const float* gamma_r,
                     const float* beta_r, const float* gamma_u, const float* beta_u, const float* h, int Hc,
                     int64_t plane, float eps, int fast, float* rh, float* u, d3d_stream_t stream);
int d3d_gru_update_gn(const float* o, const double* stats_o, const float* gamma, const float* beta, const float* u,
                      const float* h, int Hc, int64_t plane, float eps, int fast, float* h_out, d3d_stream_t stream);
/* The same cell in two elementwise passes over 104 channel planes instead of 128 (ABI 10): the reset half alone, and the update
 * gate evaluated where it is used --
 *   d3d_gru_reset_gn:        rh = sigmoid(gn_r(gates[:Hc])) * h
 *   d3d_gru_update_gates_gn: h' = u*h + (1-u)*tanh(gn_o(o)),  u = sigmoid(gn_u(gates[Hc:]))   (gates: the whole [2Hc,plane] tensor)
 * Per element the operations of the pair above in their order: the same bits.  plane % 4 == 0 and 16-byte aligned tensors, else
 * D3D_ERR_UNSUPPORTED (nothing launched). */
int d3d_gru_reset_gn(const float* gates, const double* stats_r, const float* gamma_r, const float* beta_r, const float* h, int Hc,
                     int64_t plane, float eps, int fast, float* rh, d3d_stream_t stream);
int d3d_gru_update_gates_gn(const float* o, const double* stats_o, const float* gamma, const float* beta, const float* gates,
                            const double* stats_u, const float* gamma_u, const float* beta_u, const float* h, int Hc, int64_t plane,
                            float eps, int fast, float* h_out, d3d_stream_t stream);
/* One ConvGRUCell2 step as ONE call (ABI 10): the gate convolution with the GroupNorm statistics in its epilogue, d3d_gru_reset_gn, the
 * candidate convolution with its statistics and d3d_gru_update_gates_gn issued back to back -- the same kernels on the same operands as
 * the four entry points one by one; what goes away is the host's work between them (a RED-Net view is 352 cells).
 *   x [Cx,H,W], h [Hc,H,W] -> hout [Hc,H,W]; wg / wc = ops._pack_z2_bf16 of the gate [2Hc,Cx+Hc,3,3] / candidate [Hc,Cx+Hc,3,3] weights;
 *   stats_g [2][2], stats_o [2]: fp64, ZEROED by the caller; gates [2Hc,H,W], rh [Hc,H,W], o [Hc,H,W]: scratch.
 * Cx + Hc = 16 | 24 | 32 | 40 (W % 4 == 0) or 64 | 128 (parts of 32); H * W % 4 == 0; 16-byte aligned tensors.  D3D_ERR_UNSUPPORTED
 * otherwise, with nothing launched. */
int d3d_gru2_cell_gn_h16(const float* x, int Cx, const float* h, int Hc, int H, int W, const void* wg, const float* bg, const void* wc,
                         const float* bc, const float* gamma_r, const float* beta_r, const float* gamma_u, const float* beta_u,
                         const float* gamma_o, const float* beta_o, float eps, int fast, double* stats_g, double* stats_o, float* gates,
                         float* rh, float* o, float* hout, d3d_stream_t stream);

/* ucsnet.py:137-151 (compute_depth of UCS-Net): d3d_softargmin_conf4 plus the spread of the per-pixel distribution,
 * var_out = lamb * sqrt(sum_d softmax(cost)_d * (depth_d - depth_out)^2)  [h,w]. */
int d3d_softargmin_conf4_var(const float* cost, const float* depth, int depth_mode, int D, int h, int w, float lamb,
                             float* depth_out, float* conf_out, float* var_out, d3d_stream_t stream);

/* ucsnet.py:42-51 (uncertainty_aware_samples, stages after the first): out[d,y,x] = low + step * d + 1e-12 with
 * low = cur - var, step = ((cur + var) - low) / (D - 1); cur_depth, exp_var [h,w] -> out [D,h,w].  (The first stage's
 * uniform hypotheses, ucsnet.py:33-41, are d3d_depth_range_samples in per-plane mode: the same formula.) */
int d3d_uncertainty_samples(const float* cur_depth, const float* exp_var, int D, int h, int w, float* out,
                            d3d_stream_t stream);

/*
 * adamvs.py:478-486 -- per-pair softmax over D, view weight = max_D prob,
 * pair depth = SUM_D prob*d.  score [D,h,w], depth [D] or [D,h,w].
 */
int d3d_pair_softmax_max(const float* score, const float* depth, int depth_mode, int D, int h, int w,
                         float* view_weight, float* pair_depth, d3d_stream_t stream);

/*
 * SURVEY.md §8f row N1 -- the consumer of the depth / confidence maps: geometric consistency between a reference
 * and a source view, and the fusion accumulators of one reference view.
 *
 * d3d_consistency_check replaces ConsistencyChecker.check (fuse/consistency_check_n.py:141-147 -> check_cupy
 * :29-138): reference pixel -> source pixel (nearest, "+0.5 truncate"; out-of-range indices wrap around as CuPy's
 * integer-array indexing does), sampled source depth -> world -> reference pixel; a pixel is consistent when the
 * reprojection distance < position_threshold, |d_reproj - d_ref| / d_ref < depth_threshold, the reference
 * confidence > confidence_threshold, the cosine between the world normals > normal_cos_threshold
 * (= cos(radians(normal_threshold)), :22) and d_ref > 0.
 *   depth_ref, prob_ref [H,W]; normal_ref [H,W,3]; depth_src [Hs,Ws]; normal_src [Hs,Ws,3]   (device, fp32)
 *   cam: HOST array of D3D_FUSION_CAM_DOUBLES doubles, every matrix row-major and computed in float32 as the
 *        reference does (linalg.inv / matmul of float32 arrays), then widened:
 *          inv(K_ref)[9], (E_src @ inv(E_ref))[:3,:4][12], K_src[9], inv(K_src)[9], inv(E_src)[16],
 *          E_ref[:3,:4][12], K_ref[9], inv(E_src[:3,:3])[9], inv(E_ref[:3,:3])[9]
 *   outputs (device; any may be NULL): mask [H,W] u8; depth_reprojected [H,W] (0 where inconsistent);
 *        depth_src_out [Hs,Ws]: a COPY of depth_src made by the caller, in which the samples of consistent pixels
 *        are set to 0 (:123-126); xyz_world_src [3,H,W] and angle_conf [3,H,W] (cosine, clamped at 0; 0 where
 *        inconsistent).
 *
 * d3d_fusion_ref_init / _accumulate / _finalize are the body of Fuse_Depth_Map.fuse_depths for one reference view
 * (fuse/fusion_3d_normal.py:452-474, :476-518, :522-527) on resident accumulators: all_xyz_world [3,H,W],
 * conf_sum [H,W] (the reference's three identical planes kept once), geo_mask_sum [H,W] i32, vis [H,W] i32
 * (= mask * src_idx, :518).  _accumulate is the consistency check fused with :513-518 -- the pair outputs never
 * reach memory.  For _ref_init the cam slots inv(K_ref), inv(E_src) (holding inv(E_ref)) and inv(E_ref[:3,:3])
 * are read; normal_world [H,W,3] (unit world normals, :466-469) may be NULL.
 */
#define D3D_FUSION_CAM_DOUBLES 94
int d3d_consistency_check(const float* depth_ref, const float* normal_ref, const float* prob_ref,
                          const float* depth_src, const float* normal_src, const double* cam, int H, int W, int Hs,
                          int Ws, double position_threshold, float depth_threshold, float normal_cos_threshold,
                          float confidence_threshold, unsigned char* mask, float* depth_reprojected,
                          float* depth_src_out, float* xyz_world_src, float* angle_conf, d3d_stream_t stream);
int d3d_fusion_ref_init(const float* depth_ref, const float* normal_ref, const double* cam, int H, int W,
                        float* all_xyz_world, float* conf_sum, int* geo_mask_sum, float* normal_world,
                        d3d_stream_t stream);
int d3d_fusion_accumulate(const float* depth_ref, const float* normal_ref, const float* prob_ref,
                          const float* depth_src, const float* normal_src, const double* cam, int H, int W, int Hs,
                          int Ws, double position_threshold, float depth_threshold, float normal_cos_threshold,
                          float confidence_threshold, int src_idx, int* geo_mask_sum, float* all_xyz_world,
                          float* conf_sum, int* vis, float* depth_src_out, d3d_stream_t stream);
int d3d_fusion_finalize(const float* all_xyz_world, const float* conf_sum, const int* geo_mask_sum, int H, int W,
                        int min_geo_consist_num, float* avg_xyz_world, unsigned char* final_mask, d3d_stream_t stream);

/*
 * fuse/fusion_3d_normal.py:545-570 -- the confirmed pixels of a reference view as point-cloud vertices, replacing the
 * boolean-index compaction and the Python loop over points.  Two calls, because the caller sizes the outputs:
 *   d3d_fusion_mark_points: pixel i is KEPT iff final_mask[i], its ordinal among the valid pixels (row-major) is a
 *     multiple of skip_line, and scene_range_xy[0] < x < [1] and [2] < y < [3] (host array of 4 doubles; strict, NaN fails).
 *     keep [H*W] bytes; counts[0] = valid pixels, counts[1] = kept points (device, read them after the stream).
 *   d3d_fusion_gather_points: out_xyz [n,3], out_color [n,3] = trunc(color * 255) of color [H,W,3] in 0..1 (NULL: skipped),
 *     out_normal [n,3] of normal_world [H,W,3] (NULL: skipped), out_views [n,n_vis] = sorted(vis[vis > 0] - 1) padded
 *     with -1, out_nviews [n]; rows in the order of the reference's lists.  vis: HOST array of n_vis device pointers.
 *   scratch: d3d_fusion_points_scratch_bytes(H, W) bytes of device memory shared by both calls (caller-owned).
 */
size_t d3d_fusion_points_scratch_bytes(int H, int W);
int d3d_fusion_mark_points(const float* avg_xyz_world, const unsigned char* final_mask, int H, int W, int skip_line,
                           const double* scene_range_xy, void* scratch, unsigned char* keep, unsigned* counts,
                           d3d_stream_t stream);
int d3d_fusion_gather_points(const float* avg_xyz_world, const unsigned char* keep, const int* const* vis, int n_vis,
                             const float* color, const float* normal_world, int H, int W, void* scratch, float* out_xyz,
                             int* out_color, float* out_normal, int* out_views, int* out_nviews, d3d_stream_t stream);


/*
 * SURVEY.md §8f row N2 -- PFM payload order.  save_pfm_utf8 (mvs/mvs_cas/datasets/data_io.py:196-223) writes rows
 * bottom-up (np.flipud) and read_pfm / load_pfm (data_io.py:150-193, IO/pfm.py:19-60) flips them back.
 * d3d_flip_rows: out[k][H-1-y][x] = maps[k][y][x] for n <= 8 maps [H,W] (maps: HOST array of device pointers; out
 * [n,H,W] device, must not alias an input): one staging buffer in file order for a single D2H copy, or the
 * inverse after an upload.
 */
int d3d_flip_rows(const float* const* maps, int n, int H, int W, float* out, d3d_stream_t stream);

/*
 * SURVEY.md §8f row N3 -- input side of a view: crop window + per-image normalisation of a decoded 8-bit image, as
 * the dataset item builder does for every view (mvs/mvs_cas/datasets/preprocess.py:60-88 crop_input, :92-117
 * center_image; cas_normal_eval.py:112-147).
 *   img [h,w,channels] u8 interleaved (device); window rows y0..y0+H, columns x0..x0+W; out [channels,H,W] fp32.
 *   mode 0 'standard': x / 255;  mode 1 'mean': (x - mean_c) / (sqrt(var_c) + 1e-8) with the population mean and
 *   variance of channel c over the window (exact integer sums, evaluated in double, applied in float32);
 *   mode 2 'vit' (3 channels): (x - {123.675, 116.28, 103.53}_c) / ({58.395, 57.12, 57.375}_c + 1e-8).
 *   sums: device workspace of 8 uint64 (zeroed by the call, stream-ordered).
 */
int d3d_center_image_u8(const unsigned char* img, int h, int w, int channels, int y0, int x0, int H, int W, int mode,
                        unsigned long long* sums, float* out, d3d_stream_t stream);

/*
 * DESIGN.md §1 row N5 -- surface normals from depth: ComputeNormals.compute_normal_by_depth (mvs/mvs_cas/models/
 * compute_normals.py:32-82; the reference defines it and never calls it), the producer of the {view}_normal.pfm that
 * the fusion step reads (fuse/fusion_3d_normal.py:437-443, 491-498; read_normal :191-195 decodes x * 2 - 1).
 *   depth [B,H,W] fp32 (device); kinv: HOST array of B x 9 fp32, inv(K) of every item row-major, the caller's fp32
 *   inverse (the reference's torch.inverse(intrinsics), :23).  Per pixel at distance >= nei from every border, P = inv(K) (x d, y d, d); the
 *   eight differences of the 3x3 stencil of step nei against the centre with the reference's signs (:51-58), the four
 *   cross products (x1, y1), (x0, y0), (x0y1, x0y0), (x1y0, x1y1), each normalised (F.normalize: v / max(|v|, 1e-12)),
 *   summed, normalised again.  The border band of width nei is 0 (:80); a map with H == 2 nei or W == 2 nei is all 0.
 *   normal [B,H,W,3] interleaved (the layout d3d_fusion_* read); encoded [B,H,W,3] = (normal + 1) / 2, the payload of
 *   {view}_normal.pfm.  Either output may be NULL, not both.  nei < 1, H < 2 nei or W < 2 nei: D3D_ERR_INVALID_ARG.
 * The differences are formed as d_a inv(K) (dx, dy, 0) + (d_a - d_c) inv(K) (x, y, 1) -- the same quantity without the
 * cancellation of two fp32 points (csrc/normals.hip); fp32, no atomics: bit-reproducible, and item b of a batched call
 * equals a call on item b alone.
 */
int d3d_normals_from_depth(const float* depth, const float* kinv, int B, int H, int W, int nei, float* normal,
                           float* encoded, d3d_stream_t stream);

/*
 * DESIGN.md §4.8 -- digital surface model from a point cloud: the product of the reference's CREATEDSM step with
 * dsm_source "pc" (run.py:209-247 calls pc2dsm.DSM_from_PC, which the reference never shipped; the semantics are this
 * project's, deep3d_aerial_amd/dsm.py).
 *   xyz [n_points,3] fp32 (device), n_points < 2^31; a W x H raster, W * H < 2^31, row 0 north: the cell of a point is
 *   j = floor((x - x_min) / unit_x), i = floor((y_max - y) / unit_y), in fp64 with IEEE division.  A point is kept when
 *   x, y, z are finite, 0 <= i < H, 0 <= j < W and z_min <= z <= z_max (pass -inf / +inf for no height bounds).
 *   count [H,W] int32: the kept points per cell.  height [H,W] fp32: NaN where count < max(min_points, 1), else
 *   select 0 (Max): the largest z; select 1 (Robust_Max): with the cell's n heights in descending IEEE total order
 *   (-0.0 < +0.0), the (t+1)-th, t = floor(trim * n) (fp64), trim in [0, 1).
 *   scratch: device memory of d3d_dsm_scratch_bytes(n_points, W, H, select) bytes (0 for an out-of-range argument).
 *   Integer atomics and fixed-order selection only: the rasters are bit-identical for any order or split of the points.
 */
size_t d3d_dsm_scratch_bytes(long long n_points, int W, int H, int select);
int d3d_dsm_from_points(const float* xyz, long long n_points, double x_min, double y_max, double unit_x, double unit_y,
                        double z_min, double z_max, int W, int H, int select, double trim, int min_points, void* scratch,
                        size_t scratch_bytes, float* height, int* count, d3d_stream_t stream);

/*
 * DESIGN.md §4.8 -- the MovingAverage hole fill of a DSM raster (pc_interpolation_method), one pass:
 *   out = in where in is not NaN; a NaN cell gets the mean of the non-NaN cells of the (2 radius + 1)^2 window around it,
 *   clipped to the raster, summed in fp64 in the order dy = -radius..radius (outer), dx = -radius..radius (inner), divided
 *   by their number and rounded once to fp32; NaN when the window holds none.  radius in 1..16; in and out [H,W] fp32
 *   (device), not overlapping.  Iterations are repeated calls, each reading the previous output.
 */
int d3d_dsm_fill_moving_average(const float* in, float* out, int W, int H, int radius, d3d_stream_t stream);

/*
 * DESIGN.md §4.35 -- bare-earth terrain (DTM) and object heights (nDSM) from a DSM raster.  The rule is this project's
 * (deep3d_aerial_amd/dtm.py states it in full); the reference has no DTM.  Every raster is [H,W] fp32 (device), NaN = empty,
 * W * H < 2^31; every NaN written is 0x7fc00000.
 *   d3d_dtm_erode: out[i,j] = the smallest non-NaN value of rows i-ry..i+ry, columns j-rx..j+rx of `in`, clipped to the raster,
 *   in the IEEE total order (-0.0 < +0.0); NaN when the window holds none.  d3d_dtm_dilate: the largest.  d3d_dtm_open:
 *   dilate(erode(in)).  rx, ry in 1..D3D_DTM_MAX_RADIUS.  Exact selections: the result depends on no launch shape.  The work and
 *   the bytes moved per cell do not depend on the radius (running extremes over segments of 2 r + 1 cells, csrc/dtm.hip).
 *   scratch: device memory of d3d_dtm_scratch_bytes(W, H) bytes (two rasters; 0 for an out-of-range size); in, out and
 *   scratch do not overlap.
 *   d3d_dtm_classify, level k in 1..254: a cell is struck when fp32(surface - opened) > dh (false when either is NaN).  k == 1
 *   writes every cell of level: 255 where surface is NaN, else 1 when struck, else 0.  k > 1 writes k into the struck cells
 *   whose level is 0 and leaves the others.
 *   d3d_dtm_ground: ground = height where level == 0, else NaN.  d3d_dtm_ndsm: ndsm = fp32(height - dtm), NaN where either is.
 *   d3d_dtm_pull: coarse [ceil(Hf/2), ceil(Wf/2)]; a coarse cell (I, J) is the mean of its non-NaN children (2I+a, 2J+b) in
 *   range, summed in fp64 in the order (a, b) = (0,0), (0,1), (1,0), (1,1), divided by their number, rounded once; NaN with none.
 *   d3d_dtm_push: a NaN cell (i, j) of fine gets fp32(sum(w v) / sum(w)) in fp64 over the coarse cells (I0, J0) w 9, (I0, J1) w 3,
 *   (I1, J0) w 3, (I1, J1) w 1, in that order, I0 = i >> 1, I1 = I0 + (i odd ? 1 : -1), J alike; coarse cells out of range or
 *   NaN are skipped, NaN with none.  Cells of fine that hold a value are not written.  fine and coarse do not overlap.
 * No atomics: every output is the same bits run to run.
 */
#define D3D_DTM_MAX_RADIUS 1024
size_t d3d_dtm_scratch_bytes(int W, int H);
int d3d_dtm_erode(const float* in, float* out, int W, int H, int rx, int ry, void* scratch, size_t scratch_bytes,
                  d3d_stream_t stream);
int d3d_dtm_dilate(const float* in, float* out, int W, int H, int rx, int ry, void* scratch, size_t scratch_bytes,
                   d3d_stream_t stream);
int d3d_dtm_open(const float* in, float* out, int W, int H, int rx, int ry, void* scratch, size_t scratch_bytes,
                 d3d_stream_t stream);
int d3d_dtm_classify(const float* surface, const float* opened, float dh, int k, unsigned char* level, int W, int H,
                     d3d_stream_t stream);
int d3d_dtm_ground(const float* height, const unsigned char* level, float* ground, int W, int H, d3d_stream_t stream);
int d3d_dtm_ndsm(const float* height, const float* dtm, float* ndsm, int W, int H, d3d_stream_t stream);
int d3d_dtm_pull(const float* fine, int Wf, int Hf, float* coarse, d3d_stream_t stream);
int d3d_dtm_push(const float* coarse, float* fine, int Wf, int Hf, d3d_stream_t stream);

/*
 * DESIGN.md §4.36 -- the objects of an nDSM raster: connected components of its foreground, their statistics and the label
 * raster.  The rule is this project's (deep3d_aerial_amd/objects.py states it in full); the reference has no such step.
 * Every raster is [H,W] (device), W * H < 2^31 - 1; a cell's linear index is i * W + j.
 *   d3d_objects_foreground: a cell is foreground when ndsm is finite and ndsm >= min_height (an IEEE compare; NaN is not).
 *   mask (uint8, 0 / 1) and maskf (fp32, 0.0 / 1.0) get it; either may be null, not both.
 *   d3d_objects_label: exactly one of ndsm (fp32, the predicate above) and mask (uint8, nonzero = foreground) is given.
 *   connectivity 4 or 8.  parent [H,W] int32 gets -1 for background and, for a foreground cell, the smallest linear index of
 *   its component (its root): a minimum, so it depends on no order of unions and no tile size.  Tiles of D3D_OBJECTS_TILE
 *   cells square are labelled in LDS, the pairs across tile edges joined in parent by a lock-free find-and-atomicMin loop
 *   bounded by strictly decreasing parents, one pass then sets every cell to its root.  counters (device, two int64, or null)
 *   gets the number of hooks and of repeated passes of that loop.
 *   scratch of d3d_objects_scratch_bytes(W, H) bytes (0 for an out-of-range size) holds the provisional ids between the next
 *   three calls, which take the same scratch unchanged:
 *   d3d_objects_roots: the roots in index order get the provisional ids 0 .. *n_roots - 1 (device int64).
 *   d3d_objects_stats: acc [n_roots, D3D_OBJECTS_SLOTS] int64 per provisional id: cells, sum_i, sum_j, hsum, i0, i1, j0, j1, the
 *   dsm_key of the largest ndsm; hsum sums q(h) = min(2^32 - 1, floor(fp64(h) * 1024 + 0.5)).  The entry point initialises acc.
 *   d3d_objects_relabel: a component is kept when cells >= min_cells (>= 1); the kept ones get the ids 1 .. *n_kept in index
 *   order; final_id [n_roots] int32 gets the number of kept components before each; label [H,W] int32 gets the id of the cell's
 *   component, 0 for background and dropped components.
 * Integer atomics only: every output is the same bits run to run.
 */
#define D3D_OBJECTS_TILE 64
#define D3D_OBJECTS_SLOTS 9
size_t d3d_objects_scratch_bytes(int W, int H);
int d3d_objects_foreground(const float* ndsm, float min_height, unsigned char* mask, float* maskf, int W, int H, d3d_stream_t stream);
int d3d_objects_label(const float* ndsm, float min_height, const unsigned char* mask, int connectivity, int* parent, int W, int H,
                      long long* counters, d3d_stream_t stream);
int d3d_objects_roots(const int* parent, int W, int H, void* scratch, size_t scratch_bytes, long long* n_roots, d3d_stream_t stream);
int d3d_objects_stats(const float* ndsm, const int* parent, int W, int H, const void* scratch, size_t scratch_bytes, long long n_roots,
                      long long* acc, d3d_stream_t stream);
int d3d_objects_relabel(const int* parent, const long long* acc, long long n_roots, long long min_cells, int* final_id, int* label,
                        int W, int H, void* scratch, size_t scratch_bytes, long long* n_kept, d3d_stream_t stream);

/*
 * DESIGN.md §4.37 -- the outlines of a label raster: the boundary rings of every object as lattice vertices.  The rule is this
 * project's (deep3d_aerial_amd/outlines.py states it in full); the reference has no such step.
 * label [H,W] int32 (device): 0 background, ids > 0 objects; 1 <= W * H <= D3D_OUTLINES_MAX_CELLS, so there are fewer than 2^31
 * unit edges; cells outside the raster count as 0.  Corner (i, j) is the upper-left corner of cell (i, j).  A cell c with label
 * L > 0 has one directed unit edge, the cell on its left, on every side s whose neighbour is not L: 0 top (i, j+1) -> (i, j),
 * 1 left (i, j) -> (i+1, j), 2 bottom (i+1, j) -> (i+1, j+1), 3 right (i+1, j+1) -> (i, j+1).  The slot of an edge is its rank
 * in (i * W + j, s) order; its key is (i * W + j) * 4 + s.  Successor of (c, s), d its direction, o the neighbour offset of s,
 * la / ra whether c + d / c + d + o hold L: connectivity 8: ra -> (c + d + o, s - 1), else la -> (c + d, s), else (c, s + 1);
 * connectivity 4: not la -> (c, s + 1), else not ra -> (c + d, s), else (c + d + o, s - 1).  The edges fall into closed rings; a
 * ring's leader is its smallest slot, the rings are ordered by leader, and a ring's vertices are the heads of its corner edges
 * (the successor has another side) in ring order from the leader.
 *   scratch of d3d_outlines_scratch_bytes(W, H) bytes (0 for an out-of-range size) serves every call that takes one.
 *   d3d_outlines_count: offset [H,W] int32 gets every cell's first slot; counters (device, two int64) the number of edges and a
 *   nonzero word when a label is negative (such cells count as background; the Python layer refuses them).
 *   d3d_outlines_edges: per slot, succ the successor's slot, key the key, state (16 bytes per edge) the start of the ranking,
 *   (m, dm, nx) = (slot, 0, succ).  n_edges is the count's total, 1 .. 4 W H.
 *   d3d_outlines_rank: round k (0 .. 30) of the pointer jumping from state_in to state_out: t = nx[e]; if m[t] < m[e] then
 *   m[e] = m[t] and dm[e] = 2^k + dm[t]; nx[e] = nx[t].  changed (device int32) is cleared and then set when an m changed.  The
 *   round that changes none is the last: m is then the ring's leader and dm the hops to it.
 *   d3d_outlines_rings: ring_id [n_edges] int32 gets the number of leaders below each slot; *n_rings (device int64) their number.
 *   d3d_outlines_place: ring_len, ring_edge, ring_object [n_rings] int32 get each ring's length 1 + dm[succ[leader]], the sum of
 *   the lengths before it and its label; ordered [n_edges] gets the keys in ring order, edge e at
 *   ring_edge + (len - dm[e]) mod len, bit 31 set on a corner edge; corner [n_edges] int32 the number of corner edges before
 *   each place; *n_vertices (device int64) their number.
 *   d3d_outlines_emit: vertices [n_vertices,2] int32 gets the head (i, j) of every corner edge, ring_start [n_rings + 1] int32
 *   each ring's first vertex and n_vertices.
 * No float and no order of execution enters any output: the same bits run to run.
 */
#define D3D_OUTLINES_MAX_CELLS 536870911
size_t d3d_outlines_scratch_bytes(int W, int H);
int d3d_outlines_count(const int* label, int W, int H, int* offset, void* scratch, size_t scratch_bytes, long long* counters,
                       d3d_stream_t stream);
int d3d_outlines_edges(const int* label, const int* offset, int connectivity, int W, int H, long long n_edges, int* succ, int* key,
                       int* state, d3d_stream_t stream);
int d3d_outlines_rank(const int* state_in, int* state_out, long long n_edges, int round, int* changed, d3d_stream_t stream);
int d3d_outlines_rings(const int* state, int W, int H, long long n_edges, int* ring_id, void* scratch, size_t scratch_bytes,
                       long long* n_rings, d3d_stream_t stream);
int d3d_outlines_place(const int* label, int W, int H, const int* state, const int* succ, const int* key, const int* ring_id,
                       long long n_edges, long long n_rings, int* ring_len, int* ring_edge, int* ring_object, unsigned* ordered,
                       int* corner, void* scratch, size_t scratch_bytes, long long* n_vertices, d3d_stream_t stream);
int d3d_outlines_emit(const unsigned* ordered, const int* corner, const int* ring_edge, int W, int H, long long n_edges,
                      long long n_rings, long long n_vertices, int* vertices, int* ring_start, d3d_stream_t stream);

/*
 * DESIGN.md §4.11 -- digital surface model from a triangle mesh: the reference's CREATEDSM step with dsm_source "mesh"
 * (run.py:226-232 calls mesh2dsm.DSM_from_Mesh, which the reference never shipped; the semantics are this project's,
 * deep3d_aerial_amd/dsm.py).  The raster is the one of d3d_dsm_from_points.
 *   vertices [n_vertices,3] fp32 and faces [n_faces,3] int32 (device), both counts < 2^31.  Cell (i, j) samples its centre
 *   (x_min + (j + .5) unit_x, y_max - (i + .5) unit_y) in fp64.  A face is used when its indices are in range and its nine
 *   coordinates finite (others are skipped; the Python layer refuses out-of-range indices), its vertices put in lexicographic
 *   (x, y, z) order.  Edge p -> q, endpoints (u, v) in lexicographic (x, y) order, s = +1 if (u, v) == (p, q) else -1:
 *   E(p, q, P) = s ((v.x - u.x)(P.y - u.y) - (v.y - u.y)(P.x - u.x)), fp64, no contraction.  D = E(a, b, c); a face with D 0
 *   or not finite contributes nothing.  w_a = sigma E(b, c, P), w_b = sigma E(c, a, P), w_c = sigma E(a, b, P), sigma = sign(D);
 *   the centre is covered when every w >= 0 and W = (w_a + w_b) + w_c > 0; the sample fp32(((w_a z_a + w_b z_b) + w_c z_c) / W)
 *   is kept when z_min <= z <= z_max.  Only centres in the face's range are tested: columns floor((x_lo - x_min) / unit_x) - 1
 *   .. floor((x_hi - x_min) / unit_x) + 1, rows floor((y_max - y_hi) / unit_y) - 1 .. floor((y_max - y_lo) / unit_y) + 1 of its
 *   XY box, clipped to the raster.  height [H,W] fp32: the largest sample in IEEE total order, NaN where there is none.
 *   scratch: device memory of d3d_dsm_mesh_scratch_bytes(n_faces, W, H) bytes (0 for an out-of-range argument), not
 *   overlapping height.  Integer atomics only: the raster depends on the set of faces, not on their order or winding.
 */
size_t d3d_dsm_mesh_scratch_bytes(long long n_faces, int W, int H);
int d3d_dsm_from_mesh(const float* vertices, long long n_vertices, const int* faces, long long n_faces, double x_min, double y_max,
                      double unit_x, double unit_y, double z_min, double z_max, int W, int H, void* scratch, size_t scratch_bytes,
                      float* height, d3d_stream_t stream);

/*
 * DESIGN.md §4.26 -- orthophoto of the textured mesh: the mesh seen top-down on a raster, coloured from its texture atlas.  The
 * rule is this project's (deep3d_aerial_amd/ortho_mesh.py); it does not claim to match OpenMVS's orthographic image.
 *   Grid and coverage: the raster, the cell centres, the lexicographic vertex order, the fp64 edge functions and inclusive test,
 *   the degenerate and vertical rejection, the cell ranges and the sample z = fp32(((w_a z_a + w_b z_b) + w_c z_c) / W) kept
 *   when z_min <= z <= z_max are exactly those of d3d_dsm_from_mesh above (one copy of the code).
 *   Texcoords: texcoord [n_faces,6] fp32 (s, t per corner) and texnumber [n_faces] int32, as d3d_texture_texcoords writes them;
 *   they travel with the vertices through the lexicographic sort, so nothing depends on the winding or on which corner comes
 *   first.  At a covered centre s = ((w_a s_a + w_b s_b) + w_c s_c) / W in fp64, t alike; the texel position on page
 *   k = texnumber is x = s page_width - 0.5, y = (1 - t) h_k - 0.5, h_k = page_row[k + 1] - page_row[k] (the inverse of
 *   d3d_texture_texcoords).
 *   Colour: the bilinear tap of d3d_ortho_colorize on page k at (x, y) -- x0 = floor(x) clamped to the page, fx = x - floor(x),
 *   x1 = min(x0 + 1, page_width - 1), y alike, the weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy summed in that order in
 *   fp64 --, each channel floor(c + 0.5) clamped to 0..255, alpha 255 (the atlas's own alpha is not read).  A face is untextured
 *   when its three texcoord pairs are equal bit for bit (what d3d_texture_texcoords writes for a face no view sees), its
 *   texnumber is outside 0 .. n_pages - 1 or a texcoord is not finite; it still occludes, and its colour word is 0.
 *   Which face wins: a cell keeps the largest 64-bit key (zk << 32) | colour word (R in the low byte); zk = key(z), the
 *   order-preserving fp32 -> uint32 key of the DSM, or ~key(z) when z_down is 1 (the lowest sample wins: the cameras are on
 *   the low-Z side).  No finite z has zk 0 in either mode; key 0 is the empty cell.  Equal heights (coincident faces, shared
 *   edges that round alike) go to the larger colour word, so a textured face beats an untextured one there.  The raster is a
 *   function of the set of (triangle, texcoords, page texels), never of the face order: every update is one 64-bit integer max.
 *   Outputs: rgba [H,W] RGBA8 words, 0 in empty cells and where an untextured face is on top; height [H,W] fp32, the winning
 *   sample, NaN where empty -- with z_down 0 the raster of d3d_dsm_from_mesh on the same grid, bit for bit.
 *   atlas: all pages as [page_row[n_pages], page_width] RGBA8 words (device); page_row [n_pages + 1] int64 in DEVICE memory,
 *   increasing from 0 (the host cannot read it: a page whose rows are not increasing inside 0 .. page_row[n_pages] is treated
 *   as untextured, and the Python layer refuses such an array).  scratch: device memory of
 *   d3d_ortho_mesh_scratch_bytes(n_faces, W, H) bytes (0 for an out-of-range argument: 8 bytes per cell plus the list of large
 *   faces), zeroed by the call on the stream; rgba, height and scratch must not overlap.  Null pointers, counts >= 2^31,
 *   W * H >= 2^31, a short scratch, n_pages < 1, page_width < 1, z_down outside {0, 1}: D3D_ERR_INVALID_ARG before any launch.
 */
size_t d3d_ortho_mesh_scratch_bytes(long long n_faces, int W, int H);
int d3d_ortho_from_mesh(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* texcoord,
                        const int* texnumber, const unsigned* atlas, const long long* page_row, int n_pages, int page_width,
                        double x_min, double y_max, double unit_x, double unit_y, double z_min, double z_max, int W, int H, int z_down,
                        void* scratch, size_t scratch_bytes, unsigned* rgba, float* height, d3d_stream_t stream);

/*
 * DESIGN.md §4.27 -- voxel-grid merge of the fused points into one de-duplicated cloud with colour, normal and support count.
 * The rule is this project's (deep3d_aerial_amd/cloud.py); it stands where the reference's Resample_PC would and does not claim
 * to match any tool.
 *   Grid: border = x_min, x_max, y_min, y_max, z_min, z_max (all finite, min < max) and voxel v > 0 (finite);
 *   n_a = ceil((max_a - min_a) / v) per axis, each in 1 .. 2^21 - 1.
 *   Cell of a point, per axis: u = ((double)x - min_a) / v in fp64, i = floor(u), r = floor((u - i) * 65536) in 0 .. 65535.  A
 *   point is dropped when a coordinate is not finite or an i is outside 0 .. n_a - 1 (so a point on a max face whose u equals
 *   n_a is dropped).  Key: (iz << 42) | (iy << 21) | ix, 63 bits; a dropped point gets INT64_MAX.
 *   Per occupied voxel, integer sums over its members (no grouping or order of the additions can change a bit):
 *     count, int32.
 *     Position per axis: S = sum r; min_a + (i + (S + 0.5 count) / (65536.0 count)) * v in fp64, each operation rounded once
 *     (no fused multiply-add), then rounded to fp32: within v / 65536 plus one fp32 ulp of the exact mean.
 *     Normal (normal not null): per component llrint(n_c * 2^20) as int64 is summed; a member whose normal has a non-finite
 *     component, or one of magnitude above 1024 (so 2^31 members cannot overflow), adds nothing.  Output sum / |sum| in fp64,
 *     |sum| = sqrt((x x + y y) + z z), rounded to fp32; (0, 0, 0) when the sum vector is zero.
 *     Colour (color not null; int32 [n,3], each channel clamped to 0 .. 255 on input): (2 sum + count) / (2 count) in
 *     integers, uint8 (.5 rounds up).
 *   Isolated voxels: a voxel is kept when the counts of its 3 x 3 x 3 neighbourhood (itself included; neighbours outside the
 *   grid do not exist) sum to at least min_points >= 1, over the unfiltered voxel set, in one pass.  1 keeps every voxel.
 *   Order: the kept voxels come out in increasing key.  The output is a function of the multiset of input points.
 * Every pointer is DEVICE memory.  The calls, in order (the host reads two counts: *n_voxels and *n_kept):
 *   d3d_cloud_keys: keys [n] int64 and frac [n] int64 = r_x | r_y << 16 | r_z << 32 (0 for a dropped point) of xyz [n,3] fp32.
 *   The caller sorts the keys and keeps the order (sorted_keys [n], order [n] int64: sorted_keys[i] = keys[order[i]]).
 *   d3d_cloud_heads: vox [n] int32 = the voxel of every sorted point (the number of distinct keys below its own; n_voxels for a
 *     dropped point) and *n_voxels int64 = the number of distinct keys other than INT64_MAX.
 *   d3d_cloud_accumulate: ukeys [n_voxels] int64 (increasing), count [n_voxels] int32 and acc [n_voxels, 3 + 3 (normal != null)
 *     + 3 (color != null)] int64 = S, then the normal sums, then the colour sums; count and acc are zeroed by the call on the
 *     stream.  normal [n,3] fp32 and color [n,3] int32 are indexed like xyz (through order) and may be null.
 *   d3d_cloud_neighbours: keep [n_voxels] int32 (1 or 0), pos [n_voxels] int32 = the exclusive scan of keep, *n_kept its total.
 *     nx, ny, nz: the grid's n_a.
 *   d3d_cloud_finalize: xyz [n_kept,3] fp32, normal [n_kept,3] fp32, color [n_kept,3] uint8, count [n_kept] int32 of the kept
 *     voxels; normal and color null exactly where they were null for d3d_cloud_accumulate (the width of acc follows them).
 *   scratch (heads, neighbours): d3d_cloud_scratch_bytes(n) bytes for n points or n voxels (0 for n outside 0 .. 2^31 - 1).
 * Integer atomicAdd only.  Null pointers (where the count is not 0), counts outside 0 .. 2^31 - 1, n_voxels > n_points,
 * n_kept > n_voxels, a bad border, voxel or grid, min_points < 1, a short scratch, overlapping buffers: D3D_ERR_INVALID_ARG
 * before any launch.
 */
size_t d3d_cloud_scratch_bytes(long long n);
int d3d_cloud_keys(const float* xyz, long long n_points, double x_min, double x_max, double y_min, double y_max, double z_min,
                   double z_max, double voxel, long long* keys, long long* frac, d3d_stream_t stream);
int d3d_cloud_heads(const long long* sorted_keys, long long n_points, void* scratch, size_t scratch_bytes, int* vox,
                    long long* n_voxels, d3d_stream_t stream);
int d3d_cloud_accumulate(const long long* sorted_keys, const long long* order, const int* vox, const long long* frac,
                         const float* normal, const int* color, long long n_points, long long n_voxels, long long* ukeys, int* count,
                         long long* acc, d3d_stream_t stream);
int d3d_cloud_neighbours(const long long* ukeys, const int* count, long long n_voxels, int nx, int ny, int nz, int min_points,
                         void* scratch, size_t scratch_bytes, int* keep, int* pos, long long* n_kept, d3d_stream_t stream);
int d3d_cloud_finalize(const long long* ukeys, const int* count, const long long* acc, const int* keep, const int* pos,
                       long long n_voxels, long long n_kept, double x_min, double x_max, double y_min, double y_max, double z_min,
                       double z_max, double voxel, float* xyz, float* normal, unsigned char* color, int* out_count,
                       d3d_stream_t stream);

/*
 * DESIGN.md §4.28 -- outlier removal on a point cloud by capped k-nearest-neighbour distances.  The rule is this project's
 * (deep3d_aerial_amd/cloud_outliers.py); it does not claim to match any tool.
 *   Grid: the cloud's grid above with voxel = the radius h: one cell is one radius wide.  A point is keyed by d3d_cloud_keys,
 *   the single copy of the keying rule; a point it drops (key INT64_MAX) is unkeyed: dist = -1, nn = -1, nobody's neighbour,
 *   not in the sums.
 *   Per keyed point i, over every other keyed point j (j != i by index: a duplicate of i at distance 0 counts):
 *     d2 = (dx dx + dy dy) + dz dz in fp64, dx = (double)x_i - (double)x_j, each operation rounded once; cap2 = h h.
 *     e_ij = 1024 when d2 >= cap2, else min(1024, llrint(sqrt(d2) / h * 1024.0)).
 *     nn_i = the number of j with d2 < cap2.
 *     dist_i = D_i = the sum of the k smallest e_ij, a missing neighbour (fewer than k candidates) counting 1024: an integer in
 *     0 .. 1024 k, which neither the order nor the tie-breaking of the selection can change.  A point within h lies in the
 *     3 x 3 x 3 cells around i's cell and anything further adds exactly 1024, so the 27-cell window is the unbounded answer.
 *   sums [3] int64 = m (the keyed points), S1 = sum D, S2 = sum D^2 over them; k <= 32 and m < 2^31 keep S2 below 2^61.
 * Every pointer is DEVICE memory.  The calls, in order: d3d_cloud_keys with voxel = radius (its frac output is not used), the
 * caller's sort (sorted_keys [n], order [n] int64: sorted_keys[i] = keys[order[i]]), then
 *   d3d_cloud_outliers_distances: dist [n] int32, nn [n] int32 in the order of xyz [n,3] fp32, and sums, which the call zeroes
 *     on the stream (n_points = 0 launches nothing and writes nothing).  nx, ny, nz: the grid's n_a; k in 1 .. 32.
 *   scratch: d3d_cloud_outliers_scratch_bytes(n) bytes (0 for n outside 0 .. 2^31 - 1): the coordinates in key order.
 * The host then reads sums once and thresholds dist and nn (cloud_outliers.py).  One integer atomicAdd per workgroup and sum,
 * no other atomics.  Null pointers (where the count is not 0), a count outside 0 .. 2^31 - 1, a bad grid, radius or k, a short
 * scratch, overlapping buffers: D3D_ERR_INVALID_ARG before any launch.
 */
size_t d3d_cloud_outliers_scratch_bytes(long long n);
int d3d_cloud_outliers_distances(const float* xyz, const long long* sorted_keys, const long long* order, long long n_points, int nx,
                                 int ny, int nz, double radius, int k, void* scratch, size_t scratch_bytes, int* dist, int* nn,
                                 long long* sums, d3d_stream_t stream);

/*
 * DESIGN.md §4.29 -- comparison of two point clouds by capped nearest-neighbour distances: accuracy, completeness, F-score.  The
 * rule is this project's (deep3d_aerial_amd/cloud_compare.py); it does not claim to match any tool.
 *   Grid: the cloud's grid above with voxel = the cap h: one cell is one cap wide.  The queries Q [n_query,3] fp32 and the
 *   targets T [n_target,3] fp32 are both keyed by d3d_cloud_keys, the single copy of the keying rule; a point it drops (key
 *   INT64_MAX) is unkeyed: as a query e = -1, idx = -1 and in no count; as a target nobody's neighbour.
 *   Per keyed query i, over every keyed target j:
 *     d2 = (dx dx + dy dy) + dz dz in fp64, dx = (double)q_x - (double)t_x, each operation rounded once; cap2 = h h.
 *     The nearest is the j with d2 < cap2 that minimises (d2, j), j the index in T's input order: of equally distant targets
 *     the lowest input index wins.
 *     Found: idx_i = j and e_i = min(1024, llrint(sqrt(d2) / h * 1024.0)), the outliers' e.  None: idx_i = -1, e_i = 1024.
 *     e does not decrease with d2, so e_i does not depend on the tie rule.  A target within h lies in the 3 x 3 x 3 cells
 *     around the query's cell, so the 27-cell window is exact under the cap.
 *   hist [1026] int64: hist[e], e in 0 .. 1024, counts the keyed queries that found a neighbour with that e; hist[1025] those
 *   that found none; the sum is the number of keyed queries.
 * Every pointer is DEVICE memory.  The calls, in order: d3d_cloud_keys with voxel = cap on either cloud (its frac output is not
 * used), the caller's sort of either (sorted_keys [n], order [n] int64: sorted_keys[i] = keys[order[i]]), then
 *   d3d_cloud_compare_nearest: e [n_query] int32 and idx [n_query] int32 in the order of q_xyz, and hist, which the call zeroes
 *     on the stream.  n_query = 0 writes only the zeroed hist; n_target = 0 gives every keyed query (1024, -1) and hist[1025].
 *     nx, ny, nz: the grid's n_a.
 *   scratch: d3d_cloud_compare_scratch_bytes(n_query, n_target) bytes (0 when either count is outside 0 .. 2^31 - 1): the
 *     targets as 16-byte records {x, y, z, input index} in key order.
 * The host turns the two histograms (Q = cloud against T = reference, and the reverse) into the statistics (cloud_compare.py).
 * One integer atomicAdd per keyed query in LDS and one per workgroup and non-empty bin in memory, no other atomics.  Null
 * pointers (where the count is not 0), a count outside 0 .. 2^31 - 1, a bad grid or cap, a short scratch, overlapping buffers
 * (the two clouds' arrays included): D3D_ERR_INVALID_ARG before any launch.
 */
size_t d3d_cloud_compare_scratch_bytes(long long n_query, long long n_target);
int d3d_cloud_compare_nearest(const float* q_xyz, const long long* q_sorted_keys, const long long* q_order, long long n_query,
                              const float* t_xyz, const long long* t_sorted_keys, const long long* t_order, long long n_target, int nx,
                              int ny, int nz, double cap, void* scratch, size_t scratch_bytes, int* e, int* idx, long long* hist,
                              d3d_stream_t stream);

/*
 * DESIGN.md §4.31 -- rigid registration of a point cloud to a reference cloud (iterative closest point) around the search above:
 * the transform and the sums of the matched pairs.  The rule is this project's (deep3d_aerial_amd/cloud_register.py, which also
 * holds the closed-form solve and the iteration, host fp64); it does not claim to match any tool.
 *   d3d_cloud_transform: out [n,3] fp32 from xyz [n,3] fp32 and rt, 12 doubles in DEVICE memory, a row-major 3 x 4 matrix T.
 *     Per output row r: p'_r = (float)(((T[r][0] (double)x + T[r][1] (double)y) + T[r][2] (double)z) + T[r][3]), every operation
 *     fp64 and rounded once (no fused multiply-add), the result rounded once to fp32.  A non-finite input gives whatever that
 *     arithmetic gives.  out must not overlap xyz.  n = 0 launches nothing.
 *   d3d_cloud_register_sums: q_xyz [n_query,3] fp32 the moved cloud, e and idx [n_query] int32 what d3d_cloud_compare_nearest
 *     gave for it against t_xyz [n_target,3] fp32 on the grid of that cap whose origin is (xmin, ymin, zmin).  Pair i counts when
 *     0 <= idx_i < n_target and e_i <= e_max (an idx outside the targets is never dereferenced).  Per counted pair
 *     a_c = llrint(((double)q_c - o_c) / cap * 1024.0) and b_c likewise from t_xyz[idx_i]; a keyed point lies inside a grid of at
 *     most 2^21 - 1 cells per axis, so 0 <= a_c, b_c < 2^31 and a_r b_c < 2^62.  sums int64 [27], zeroed by the call on the
 *     stream: [0] N, the counted pairs; [1..3] sum a; [4..6] sum b; [7..15] sum (a_r b_c) & 0xFFFFFFFF, row-major; [16..24] sum
 *     (a_r b_c) >> 32; [25] sum e; [26] sum e^2.  With at most 2^31 - 1 points no slot overflows; the host recombines
 *     M_rc = hi 2^32 + lo in unbounded integers.  n_query = 0 (or n_target = 0) writes only the zeroed sums.
 * Every pointer is DEVICE memory.  One set of 27 integer atomicAdd per workgroup, no other atomics: the same bits for any order of
 * the pairs.  Null pointers (where the count is not 0), a count outside 0 .. 2^31 - 1, a non-finite origin, a cap that is not
 * finite and > 0, e_max outside 0 .. 1024, overlapping buffers: D3D_ERR_INVALID_ARG before any launch.
 */
int d3d_cloud_transform(const float* xyz, long long n, const double* rt, float* out, d3d_stream_t stream);
int d3d_cloud_register_sums(const float* q_xyz, const int* e, const int* idx, long long n_query, const float* t_xyz,
                            long long n_target, double xmin, double ymin, double zmin, double cap, int e_max, long long* sums,
                            d3d_stream_t stream);

/*
 * DESIGN.md §4.34 -- normals of a point cloud from its own neighbourhoods, and the point-to-plane sums of the registration that
 * use them.  The rules are this project's (deep3d_aerial_amd/cloud_normals.py, cloud_register.py); they do not claim to match any
 * tool.
 *   Normals.  Grid: the cloud's grid above with voxel = the radius h.  A point is keyed by d3d_cloud_keys; a point it drops is
 *   unkeyed: count 0, normal (0, 0, 0), flatness -1, nobody's neighbour.
 *   Per keyed point i the neighbours are the keyed points j, i itself included, of the 3 x 3 x 3 cells around i's cell with
 *     d2 = (dx dx + dy dy) + dz dz < h h (strict) in fp64, dx = (double)x_i - (double)x_j, each operation rounded once.
 *     Per neighbour and axis delta_c = llrint(((double)x_jc - (double)x_ic) / h * 1024.0), so |delta_c| <= 1024.
 *     Ten integer sums, int64: k (the neighbours), S1[3] = sum delta, S2[6] = sum delta_r delta_c for rc = xx xy xz yy yz zz;
 *     k < 2^31 and |S2| < 2^51, so nothing overflows and the sums are the same bits for any point order.
 *     C_rc = (double)S2_rc - ((double)S1_r * (double)S1_c) / (double)k in fp64, each operation rounded once.
 *     l0 <= l1 <= l2 and the unit eigenvector n of l0 by six cyclic Jacobi sweeps in fp64 (rotations (x, y), (x, z), (y, z) in
 *     that order, a zero off-diagonal entry skipped): n is a function of the ten integers only.  n is flipped so that
 *     n . up >= 0, up = (0, 0, 1), or (0, 0, -1) with z_down = 1; where n . up == 0 its first non-zero component is made positive.
 *     normals [n,3] fp32 = n; count [n] int32 = k; flatness [n] int32 = llrint(1024 l0 / (l0 + l1 + l2)).
 *     Degenerate -- k < 3, or l2 <= 0, or l1 <= 1e-12 l2 (collinear) --: normal (0, 0, 0), flatness -1, count k.
 *   d3d_cloud_normals: after d3d_cloud_keys with voxel = radius and the caller's sort (sorted_keys [n], order [n] int64), writes
 *     normals, count and flatness of every point in the order of xyz [n,3] fp32, and with sums_or_null not null the ten sums
 *     [n,10] int64 (k, S1 x y z, S2 xx xy xz yy yz zz) too.  n_points = 0 launches nothing.  nx, ny, nz: the grid's n_a.
 *     scratch: d3d_cloud_normals_scratch_bytes(n) bytes (0 for n outside 0 .. 2^31 - 1): the coordinates in key order.
 *     No atomics.
 *   Plane sums.  d3d_cloud_register_plane_sums: the inputs of d3d_cloud_register_sums, t_normals [n_target,3] fp32 (the normals
 *     of t_xyz) and the grid's n_a.  a, b: the bins of d3d_cloud_register_sums; c_c = 512 n_c, the grid's centre in the same
 *     units; m_c = llrint((double)normal_c * 1024.0) of the matched target.  Pair i counts when it counts there (0 <= idx_i <
 *     n_target, e_i <= e_max) and its normal is finite with every |normal_c| <= 1 and m != (0, 0, 0).  Per counted pair
 *     u = a - c, r = (a - b) . m, w = u x m, g = (w_x, w_y, w_z, m_x, m_y, m_z): the residual linearised under a rotation omega
 *     about c and a translation tau (in bins) is r + g . (omega, tau).
 *     sums int64 [87], zeroed by the call on the stream: [0] N, the counted pairs; [1] sum e; [2] sum e^2; then 28 products P_k
 *     in this order: the 21 g_i g_j, i <= j, row-major; the 6 g_i r; r r.  Each is a 128-bit two's-complement value summed in
 *     three slots 3 + 3k .. 5 + 3k: the low 32 bits of its low word, the high 32 bits of its low word (both unsigned), and its
 *     signed high word.  |w| < 2^42, |r| < 2^43, |P| < 2^87, and 2^31 - 1 pairs overflow no slot; the host recombines
 *     hi 2^64 + mid 2^32 + lo in unbounded integers.  n_query = 0 (or n_target = 0) writes only the zeroed sums.
 *     One set of 87 integer atomicAdd per workgroup, no other atomics: the same bits for any order of the pairs.
 * Every pointer is DEVICE memory.  Null pointers (where the count is not 0; sums_or_null may always be null), a count outside
 * 0 .. 2^31 - 1, a bad grid, radius, cap, origin, z_down or e_max, a short scratch, overlapping buffers: D3D_ERR_INVALID_ARG
 * before any launch.
 */
size_t d3d_cloud_normals_scratch_bytes(long long n);
int d3d_cloud_normals(const float* xyz, const long long* sorted_keys, const long long* order, long long n_points, int nx, int ny,
                      int nz, double radius, int z_down, void* scratch, size_t scratch_bytes, float* normals, int* count,
                      int* flatness, long long* sums_or_null, d3d_stream_t stream);
int d3d_cloud_register_plane_sums(const float* q_xyz, const int* e, const int* idx, long long n_query, const float* t_xyz,
                                  const float* t_normals, long long n_target, int nx, int ny, int nz, double xmin, double ymin,
                                  double zmin, double cap, int e_max, long long* sums, d3d_stream_t stream);

/*
 * DESIGN.md §4.30 -- deterministic samples of a surface mesh at a stated spacing, and a comparison's error brought back onto the
 * faces: what holds a mesh against a reference cloud with the search above.  The rule is this project's
 * (deep3d_aerial_amd/mesh_compare.py); it does not claim to match any tool.
 *   Inputs: vertices [n_vertices,3] fp32, faces [n_faces,3] int32, a spacing s, finite and > 0.
 *   Per face f with corners (A, B, C) in the face's own order, all arithmetic fp64, every operation rounded once:
 *     L2 = the largest of the three squared edge lengths, each (dx dx + dy dy) + dz dz.
 *     n_f = 0 when a corner coordinate is not finite, L2 is not a finite number > 0, or an index is outside 0 .. n_vertices - 1.
 *     Otherwise q = sqrt(L2) / s and n_f = 1 for q <= 1, else ceil(q); an n_f above 32768 is 32768 and the face counts as clipped.
 *     The face gets n_f^2 samples: the centroids of the n_f^2 congruent sub-triangles of its n_f-fold edge subdivision.
 *   Sample t (0 .. n^2 - 1) of a face with n = n_f: row r = floor(sqrt(t)) (exact), c = t - r^2 in 0 .. 2r, k = c >> 1; integer
 *     weights with p + q + w = 3n: c even: p = 3(n - r) - 2, q = 3k + 1, w = 3(r - k) + 1; c odd: p = 3(n - r) - 1, q = 3k + 2,
 *     w = 3(r - k) - 1; per axis x = ((p A_x + q B_x) + w C_x) / (3n) in fp64, then rounded to fp32.
 *   Order: (face in input order, t).  In exact arithmetic every point of a face lies within 2s/3 of a sample of that face.
 * Every pointer is DEVICE memory.  The calls, in order:
 *   d3d_mesh_sample_count: counts [n_faces] int32 = n_f^2, offsets [n_faces + 1] int32 their exclusive scan, totals int64 [2] =
 *     the samples and the clipped faces.  The offsets are valid only when totals[0] < 2^31 (the host reads totals and decides).
 *     n_faces = 0 writes the zeroed totals and offsets[0] = 0.
 *     scratch: d3d_mesh_sample_scratch_bytes(n_faces) bytes (0 for n_faces outside 0 .. 2^31 - 1): the scan's tile sums.
 *   d3d_mesh_sample_emit: xyz [n_samples,3] fp32 and face [n_samples] int32 for n_samples = totals[0], one lane per sample.
 *     n_samples = 0 launches nothing.
 *   d3d_mesh_sample_face_error: from e [n_samples] int32 of d3d_cloud_compare_nearest on the samples and face, per face
 *     sum [n_faces] int64 and keyed [n_faces] int32 over its samples with e >= 0 and worst [n_faces] int32, their maximum, -1 for
 *     a face with none.  The call zeroes sum and keyed and sets worst to -1 itself; n_samples = 0 leaves them so.
 * Integer atomicAdd and atomicMax only: one atomicAdd per workgroup and total in the count, one set per run of a face's samples
 * within a wave in the face error.  Null pointers (where the count is not 0), a count outside 0 .. 2^31 - 1, a spacing that is
 * not finite and > 0, a short scratch, overlapping buffers: D3D_ERR_INVALID_ARG before any launch.
 */
size_t d3d_mesh_sample_scratch_bytes(long long n_faces);
int d3d_mesh_sample_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, double spacing,
                          void* scratch, size_t scratch_bytes, int* counts, int* offsets, long long* totals, d3d_stream_t stream);
int d3d_mesh_sample_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* offsets,
                         long long n_samples, float* xyz, int* face, d3d_stream_t stream);
int d3d_mesh_sample_face_error(const int* e, const int* face, long long n_samples, long long n_faces, long long* sum, int* keyed,
                               int* worst, d3d_stream_t stream);

/*
 * DESIGN.md §4.9 -- true orthophoto on the DSM (the reference has no orthophoto step; the semantics are this project's,
 * deep3d_aerial_amd/ortho.py).  The grid is the DSM's: cell (i, j) is X = (x_min + (j + 0.5) unit_x, y_max - (i + 0.5) unit_y, h),
 * h = height[i,j] in fp64; a non-finite h is an empty cell.  A view is one d3d_ortho_view_t record in DEVICE memory, filled by
 * the caller: R [3,3] row-major and t of E = Tcw, K [3,3], C = -R^T t, all fp64; depth [H,W] fp32 and rgba [H,W] RGBA8 (R in
 * the low byte, one texel one 4-byte load) of the same size; id in 0 .. 2^31 - 2.
 * Projection in fp64 without contraction: p = R X + t, q = K p, each row summed left to right, u = q0 / q2, v = q1 / q2.
 * The view is a candidate for the cell when p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1, the depth D at pixel
 * (floor(v + 0.5), floor(u + 0.5)) is finite and > 0, and p2 <= D * (1 + depth_tolerance).  Its score is
 * s = (dx^2 + dy^2) / dz^2 in fp64, (dx, dy, dz) = X - C; a non-finite s rejects it.  The key is
 * (bits(fp32(s)) << 32) | id (int64); the smallest wins, the empty key is INT64_MAX.
 */
typedef struct d3d_ortho_view {
    double R[9];
    double t[3];
    double K[9];
    double C[3];
    const float* depth;
    const unsigned int* rgba;
    int W, H;
    int id;
    int pad;
} d3d_ortho_view_t;

/* d3d_ortho_select: MIN-MERGES the keys of n_views views into key [H,W] int64 (set it to INT64_MAX before the first call).
 *   height [H,W] fp32 (device), W * H < 2^31; depth_tolerance finite, >= 0; n_views < 2^20.  scratch: device memory of
 *   d3d_ortho_scratch_bytes(W, H, n_views) bytes (0 for an out-of-range argument).  A per-tile cull over the bounding box of
 *   the tile's heights only skips work.  No atomics: the key raster is bit-identical for any batching, order or split of the
 *   views. */
size_t d3d_ortho_scratch_bytes(int W, int H, int n_views);
int d3d_ortho_select(const float* height, double x_min, double y_max, double unit_x, double unit_y, int W, int H,
                     const d3d_ortho_view_t* views, int n_views, double depth_tolerance, void* scratch, size_t scratch_bytes,
                     long long* key, d3d_stream_t stream);

/* d3d_ortho_colorize: for every cell whose key's id (its low 32 bits) is the id of one of this call's views, writes
 *   rgba[i,j] = the bilinear sample of that view's image at the cell's (u, v) -- x0 = floor(u), fx = u - x0 (y alike), taps
 *   clamped to the image, weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy summed in that order in fp64, each channel
 *   floor(c + 0.5) clamped to 0..255, alpha 255 -- and view_out[i,j] = the id.  Every other cell is left untouched, so calls
 *   over disjoint view sets colour one raster together.  The (u, v) are recomputed from height and the grid, which must be
 *   the ones select ran on.  Ids must be unique within a call. */
int d3d_ortho_colorize(const float* height, double x_min, double y_max, double unit_x, double unit_y, int W, int H,
                       const long long* key, const d3d_ortho_view_t* views, int n_views, unsigned int* rgba, int* view_out,
                       d3d_stream_t stream);

/*
 * DESIGN.md §4.10 -- surface mesh from the depth maps (the reference shells out to OpenMVS; the semantics are this project's,
 * deep3d_aerial_amd/mesh.py states them in full).  A truncated signed distance field in sparse bricks of 8^3 voxels, then
 * marching tetrahedra (6 Kuhn tetrahedra per cube).  Grid: nx x ny x nz voxels of size `voxel`, voxel (i, j, k) centred at
 * (x_min + (i + 0.5) voxel, ...) in fp64; bx = ceil(nx / 8) bricks per axis (y, z alike), bx * by * bz < 2^31.  A voxel's slot
 * is brick * 512 + (lz * 8 + ly) * 8 + lx, brick its number in the allocated list.  Every pointer below is DEVICE memory
 * except `grid`, a host struct.  Integer atomics nowhere, float atomics nowhere: every pass is a fixed-order computation.
 * A view is one d3d_mesh_view_t record: R [3,3] row-major and t of E = Tcw, K [3,3] with K[1,0] = K[2,0] = K[2,1] = 0 and
 * K[2,2] = 1 (the caller checks it), depth and confidence [H,W] fp32.
 */
typedef struct d3d_mesh_grid {
    double x_min, y_min, z_min, voxel;
    int nx, ny, nz;
    int bx, by, bz;
} d3d_mesh_grid_t;

typedef struct d3d_mesh_view {
    double R[9];
    double t[3];
    double K[9];
    const float* depth;
    const float* conf;
    int W, H;
} d3d_mesh_view_t;

/* Scratch of one exclusive scan over n int32 values (8 bytes per 4096 values; 0 for n < 0).  d3d_mesh_bricks needs it for
 * n = bx * by * bz, d3d_mesh_count for n = n_bricks * 512, d3d_mesh_compact for n = n_vertices. */
size_t d3d_mesh_scan_scratch_bytes(long long n);

/* d3d_mesh_mark: one lane per pixel of each view sets marks[((bk + 1) * (by + 2) + bj + 1) * (bx + 2) + bi + 1] = 1 for the
 *   brick (bi, bj, bk) in -1 .. b of the back-projected centre of every valid pixel (depth finite and > 0, confidence >=
 *   conf_threshold).  marks: (bx + 2) (by + 2) (bz + 2) bytes, zeroed by the caller before the first batch; calls OR into
 *   it.  max_pixels >= W * H of every view. */
int d3d_mesh_mark(const d3d_mesh_grid_t* grid, const d3d_mesh_view_t* views, int n_views, int max_pixels, double conf_threshold,
                  unsigned char* marks, d3d_stream_t stream);

/* d3d_mesh_bricks: the 3 x 3 x 3 dilation of the marks, clipped to the grid, numbered in increasing linear index
 *   (bk * by + bj) * bx + bi by a reduce-then-scan.  brick_index [bz,by,bx] int32 gets the number or -1, brick_list
 *   (bx * by * bz int32) the linear index of each allocated brick, n_bricks (one int64) their count. */
int d3d_mesh_bricks(const d3d_mesh_grid_t* grid, const unsigned char* marks, void* scratch, size_t scratch_bytes, int* brick_index,
                    int* brick_list, long long* n_bricks, d3d_stream_t stream);

/* d3d_mesh_integrate: adds the views, in the order given, to sum [n_bricks * 512] fp32 and count [n_bricks * 512] int32
 *   (zeroed by the caller before the first batch).  Per voxel and view, fp64 without contraction: p = R X + t, q = K p;
 *   observed when p2 > 0, q2 > 0, pixel (floor(q1 / q2 + 0.5), floor(q0 / q2 + 0.5)) is inside and valid and
 *   sdf = D - p2 >= -trunc; then sum += fp32(min(1, sdf / trunc)), count += 1.  0 < trunc <= 8 voxel.  One workgroup per
 *   brick; views are culled per brick by the projection of its box, which only skips work. */
int d3d_mesh_integrate(const d3d_mesh_grid_t* grid, const int* brick_list, int n_bricks, const d3d_mesh_view_t* views, int n_views,
                       double trunc, double conf_threshold, float* sum, int* count, d3d_stream_t stream);

/* d3d_mesh_count: per voxel, the mask of its crossed owned edges (7 bits: +x, +y, +z, +xy, +xz, +yz, +xyz) into edges
 *   [n_bricks * 512] uint8 and the exclusive scans of their vertex and triangle counts into vert_base and face_base
 *   [n_bricks * 512] int32; totals [2] int64 gets (vertices, triangles).  The offsets are valid when both totals are below
 *   2^31.  A voxel is observed when count >= min_views (>= 1); its value is sum / count in fp32.  scratch:
 *   d3d_mesh_scan_scratch_bytes(n_bricks * 512). */
int d3d_mesh_count(const d3d_mesh_grid_t* grid, const int* brick_list, const int* brick_index, int n_bricks, const float* sum,
                   const int* count, int min_views, void* scratch, size_t scratch_bytes, unsigned char* edges, int* vert_base,
                   int* face_base, long long* totals, d3d_stream_t stream);

/* d3d_mesh_emit: the vertices [totals[0], 3] fp32 and triangles [totals[1], 3] int32 d3d_mesh_count sized, in (brick, voxel,
 *   edge type) and (brick, voxel, tetrahedron, triangle) order; referenced [totals[0]] int32, zeroed by the caller, gets 1 for
 *   every vertex a triangle uses. */
int d3d_mesh_emit(const d3d_mesh_grid_t* grid, const int* brick_list, const int* brick_index, int n_bricks, const float* sum,
                  const int* count, int min_views, const unsigned char* edges, const int* vert_base, const int* face_base,
                  float* vertices, int* faces, int* referenced, d3d_stream_t stream);

/* d3d_mesh_compact: drops the unreferenced vertices: out_vertices [n_vertices, 3] gets the referenced ones in order (the first
 *   n_kept rows), faces [n_faces, 3] are renumbered in place, remap [n_vertices] int32 is scratch, n_kept one int64.
 *   n_vertices, n_faces < 2^31; scratch: d3d_mesh_scan_scratch_bytes(n_vertices). */
int d3d_mesh_compact(const float* vertices, long long n_vertices, int* faces, long long n_faces, const int* referenced, void* scratch,
                     size_t scratch_bytes, int* remap, float* out_vertices, long long* n_kept, d3d_stream_t stream);

/*
 * DESIGN.md §4.12 -- cleaning a triangle mesh: adjacency, connected components, removal of small components and Laplacian
 * smoothing (the reference's ReconstructMesh clean options, with this project's own semantics: deep3d_aerial_amd/mesh.py states
 * them in full).  A mesh is vertices [n_vertices, 3] fp32 and faces [n_faces, 3] int32; every pointer is DEVICE memory except
 * `rounds`; faces (and vertices) may be null when there are none.  n_vertices < 2^31 and 6 n_faces < 2^31.  Faces with an index outside 0 .. n_vertices - 1 are skipped (the caller
 * refuses them).  Integer atomics only: every output is a function of the inputs, whatever the order the lanes run in.
 */
/* Scratch of d3d_mesh_adjacency (0 for out-of-range sizes). */
size_t d3d_mesh_adjacency_scratch_bytes(long long n_vertices, long long n_faces);

/* d3d_mesh_adjacency: the edges of a face are the distinct unordered pairs among (a,b) (b,c) (c,a) with unequal ends; an edge's
 *   multiplicity is the number of faces it is an edge of.  offset [n_vertices + 1] int64 and nbr (room for 6 n_faces int32,
 *   offset[n_vertices] written) get the CSR of the distinct neighbours of every vertex in increasing order; fixed [n_vertices]
 *   uint8 gets 1 where some edge of the vertex does not have multiplicity 2, or the vertex has no edge. */
int d3d_mesh_adjacency(const int* faces, long long n_faces, long long n_vertices, void* scratch, size_t scratch_bytes, long long* offset,
                       int* nbr, unsigned char* fixed, d3d_stream_t stream);

/* d3d_mesh_components: label [n_vertices] int32 gets the smallest vertex index of each vertex's component (faces connect
 *   through shared vertices; a vertex no face uses is its own component).  Hooking and pointer jumping, repeated until a
 *   hooking launch changes nothing; the host reads flag (one device int32) once per round and waits on the stream.  rounds
 *   (host, may be null) gets the number of hooking launches. */
int d3d_mesh_components(const int* faces, long long n_faces, long long n_vertices, int* label, int* flag, int* rounds, d3d_stream_t stream);

/* Scratch of d3d_mesh_component_stats (0 for an out-of-range size). */
size_t d3d_mesh_stats_scratch_bytes(long long n_vertices);

/* d3d_mesh_component_stats: per label c (a d3d_mesh_components label), face_count [n_vertices] int32 at c: the faces whose first
 *   vertex has label c; box [n_vertices, 6] fp32 at c: (min x, y, z, max x, y, z) of the vertices labelled c, NaN where no
 *   vertex has label c; diag [n_vertices] fp64: the box diagonal sqrt((dx dx + dy dy) + dz dz), d = hi - lo in fp64.
 *   global_box [6] fp32 and global_diag (one fp64) the same for every vertex some face uses (NaN when there is none). */
int d3d_mesh_component_stats(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* label,
                             void* scratch, size_t scratch_bytes, int* face_count, float* box, double* diag, float* global_box,
                             double* global_diag, d3d_stream_t stream);

/* Scratch of d3d_mesh_filter (0 for an out-of-range size). */
size_t d3d_mesh_filter_scratch_bytes(long long n_faces);

/* d3d_mesh_filter: removes the faces of component c = label[face[0]] when min_faces > 0 and face_count[c] < min_faces, or
 *   spurious > 0 and diag[c] < *global_diag / spurious (fp64).  out_faces [n_faces, 3] gets the kept faces in input order (the
 *   first *n_kept, one int64), referenced [n_vertices] int32 gets 1 for every vertex a kept face uses and 0 elsewhere: the
 *   input of d3d_mesh_compact.  min_faces >= 0, spurious finite and >= 0. */
int d3d_mesh_filter(const int* faces, long long n_faces, long long n_vertices, const int* label, const int* face_count, const double* diag,
                    const double* global_diag, long long min_faces, double spurious, void* scratch, size_t scratch_bytes, int* out_faces,
                    int* referenced, long long* n_kept, d3d_stream_t stream);

/* d3d_mesh_smooth: `iterations` Jacobi steps of the umbrella Laplacian over the CSR of d3d_mesh_adjacency.  A fixed vertex
 *   stays; any other, per component in fp32 without contraction: s = the sum of its neighbours' values in CSR order (from 0),
 *   x' = x + lambda (s / fp32(count) - x).  Each step reads the previous step's positions.  out [n_vertices, 3] gets the result,
 *   work [n_vertices, 3] is the other buffer; vertices, work and out are distinct.  0 < lambda <= 1, iterations >= 0. */
int d3d_mesh_smooth(const float* vertices, long long n_vertices, const long long* offset, const int* nbr, const unsigned char* fixed,
                    float lambda, int iterations, float* work, float* out, d3d_stream_t stream);

/*
 * DESIGN.md §4.14 -- decimating the surface mesh: memoryless quadric-error edge collapse in rounds of independent collapses
 * (the rule is this project's, deep3d_aerial_amd/mesh.py states it in full; it does not claim to match OpenMVS / VCG).  A mesh
 * is vertices [n_vertices, 3] fp32 and faces [n_faces, 3] int32, n_vertices < 2^31, 6 n_faces < 2^31.  A face with an index
 * outside 0 .. n_vertices - 1 or with a repeated index is ignored by every pass and dropped by d3d_mesh_decimate_faces (the
 * caller refuses such a mesh).  offset / nbr / fixed are d3d_mesh_adjacency's outputs for the same mesh.  The undirected edges
 * a < b are numbered in (a, b) lexicographic order; there are at most 3 n_faces, the count is a DEVICE value (n_edges) and
 * the per-edge arrays have max_edges >= n_edges entries (entries from n_edges on are written as "no candidate" or left
 * alone).  Every pointer is DEVICE memory.  All arithmetic is fp64 without contraction unless said; no float atomics; the
 * integer atomics are add and min, and their return values never reach an output.
 */
/* Scratch of d3d_mesh_decimate_incidence (0 for an out-of-range size). */
size_t d3d_mesh_decimate_incidence_scratch_bytes(long long n_vertices, long long n_faces);

/* d3d_mesh_decimate_incidence: the vertex -> face CSR.  face_offset [n_vertices + 1] int32, face_index [3 n_faces] int32: row
 *   v holds the faces with a corner at v in increasing face index. */
int d3d_mesh_decimate_incidence(const int* faces, long long n_faces, long long n_vertices, void* scratch, size_t scratch_bytes,
                                int* face_offset, int* face_index, d3d_stream_t stream);

/* d3d_mesh_decimate_quadrics: quadric [n_vertices, 10] fp64 = (aa, ab, ac, ad, bb, bc, bd, cc, cd, dd) summed over the faces of
 *   the vertex's row in row order, from 0.  A face: nrm = (p1 - p0) x (p2 - p0), len = sqrt((nx nx + ny ny) + nz nz); nothing
 *   unless len > 0; (a, b, c) = nrm / len, d = -((a x0 + b y0) + c z0), w = len / 2, each term w * (u * v). */
int d3d_mesh_decimate_quadrics(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* face_offset,
                               const int* face_index, double* quadric, d3d_stream_t stream);

/* Scratch of d3d_mesh_decimate_edges (0 for an out-of-range size). */
size_t d3d_mesh_decimate_edges_scratch_bytes(long long n_vertices);

/* d3d_mesh_decimate_edges: edges [max_edges, 2] int32 = (a, b), a < b, in lexicographic order; *n_edges (int64) their count.
 *   Edges beyond max_edges are counted but not written. */
int d3d_mesh_decimate_edges(const long long* offset, const int* nbr, long long n_vertices, void* scratch, size_t scratch_bytes,
                            long long max_edges, int* edges, long long* n_edges, d3d_stream_t stream);

/* d3d_mesh_decimate_candidates: per edge e with a free endpoint the collapse target [max_edges, 3] fp32, its cost [max_edges]
 *   fp32 and key [max_edges] int64 = (bits(cost) << 32) | (e * 2654435761 mod 2^32), or -1 when the collapse is not valid
 *   (link condition, survivor degree, flips judged at the fp32 target).  An edge with both ends fixed, and every entry from
 *   *n_edges on, gets target 0, cost 0, key -1. */
int d3d_mesh_decimate_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* offset,
                                 const int* nbr, const unsigned char* fixed, const int* face_offset, const int* face_index,
                                 const double* quadric, const int* edges, const long long* n_edges, long long max_edges, float* target,
                                 float* cost, long long* key, d3d_stream_t stream);

/* Scratch of d3d_mesh_decimate_select. */
size_t d3d_mesh_decimate_select_scratch_bytes(void);

/* d3d_mesh_decimate_select: *threshold (int64) = the k-th smallest of the keys >= 0 among key [max_edges] (the largest when
 *   there are fewer than k; -1 when k == 0 or no key is >= 0). */
int d3d_mesh_decimate_select(const long long* key, long long max_edges, long long k, void* scratch, size_t scratch_bytes,
                             long long* threshold, d3d_stream_t stream);

/* d3d_mesh_decimate_claim: claim [n_vertices] int64 = the smallest key among the eligible candidates (0 <= key <= *threshold)
 *   whose neighbourhood {a, b} U N(a) U N(b) holds the vertex (LLONG_MAX when none does); clears *n_winners. */
int d3d_mesh_decimate_claim(const long long* offset, const int* nbr, long long n_vertices, const int* edges, const long long* key,
                            const long long* n_edges, long long max_edges, const long long* threshold, long long* claim,
                            long long* n_winners, d3d_stream_t stream);

/* d3d_mesh_decimate_apply: win [max_edges] uint8 = 1 for the eligible candidates that hold the claim of every vertex of their
 *   neighbourhood.  out_vertices [n_vertices, 3] = vertices with every winner's survivor (b when only b is fixed, else a) at
 *   its target; remap [n_vertices] int32 = the survivor for a winner's other endpoint, the vertex itself otherwise;
 *   *n_winners (int64, cleared by d3d_mesh_decimate_claim) counts the winners.  vertices and out_vertices are distinct. */
int d3d_mesh_decimate_apply(const float* vertices, long long n_vertices, const long long* offset, const int* nbr, const unsigned char* fixed,
                            const int* edges, const long long* key, const float* target, const long long* n_edges, long long max_edges,
                            const long long* threshold, const long long* claim, float* out_vertices, int* remap, unsigned char* win,
                            long long* n_winners, d3d_stream_t stream);

/* Scratch of d3d_mesh_decimate_faces (0 for an out-of-range size). */
size_t d3d_mesh_decimate_faces_scratch_bytes(long long n_faces);

/* d3d_mesh_decimate_faces: out_faces = the faces through remap, without those two of whose corners meet, in input order;
 *   *n_kept (int64) their count; referenced [n_vertices] int32 = 1 for the vertices they use (for d3d_mesh_compact). */
int d3d_mesh_decimate_faces(const int* faces, long long n_faces, long long n_vertices, const int* remap, void* scratch, size_t scratch_bytes,
                            int* out_faces, int* referenced, long long* n_kept, d3d_stream_t stream);

/*
 * DESIGN.md §4.16 -- closing the small holes of the surface mesh: every boundary loop of at most max_edges edges whose faces
 * lie outside it gets a fan around one new vertex (the rule is this project's, deep3d_aerial_amd/mesh.py states it in full; it
 * does not claim to match OpenMVS / VCG).  A mesh is vertices [n_vertices, 3] fp32 and faces [n_faces, 3] int32, n_vertices <
 * 2^31, 6 n_faces < 2^31.  A face with an index outside 0 .. n_vertices - 1 or with a repeated index is ignored by every pass
 * (the caller refuses such a mesh).  Face (a, b, c) has the directed edges a->b, b->c, c->a; one is a boundary half-edge when
 * exactly one face holds its undirected edge, and that face owns it.  A vertex is simple when it has exactly one outgoing and
 * one incoming boundary half-edge.  Every pointer is DEVICE memory except `rounds`.  All arithmetic is fp64 without
 * contraction, rounded to fp32 only where said; no float atomics; the integer atomics are add, or and min, and their return
 * values never reach an output.
 */
#define D3D_MESH_HOLE_MAX_EDGES 1024

/* Scratch of d3d_mesh_holes_plan (0 for an out-of-range size). */
size_t d3d_mesh_holes_scratch_bytes(long long n_vertices);

/* d3d_mesh_boundary: face_offset / face_index are d3d_mesh_decimate_incidence's outputs for the same mesh.  boundary
 *   [3 n_faces] uint8 = 1 where corner c of face f (entry 3 f + c, the edge from corner c to corner c + 1 mod 3) is a boundary
 *   half-edge; out_count / in_count [n_vertices] int32 = the boundary half-edges leaving / entering the vertex; successor and
 *   owner [n_vertices] int32 = the head and the owning face of the vertex's outgoing boundary half-edge where out_count is 1,
 *   -1 elsewhere. */
int d3d_mesh_boundary(const int* faces, long long n_faces, long long n_vertices, const int* face_offset, const int* face_index,
                      int* out_count, int* in_count, int* successor, int* owner, unsigned char* boundary, d3d_stream_t stream);

/* d3d_mesh_boundary_loops: label [n_vertices] int32 gets the smallest vertex index of each vertex's boundary component
 *   (vertices joined by boundary half-edges; a vertex on none is its own).  count [n_vertices] int32 at a label: the
 *   component's half-edges; bad [n_vertices] int32 at a label: 1 when some vertex of the component is not simple (a component
 *   that is not bad is one cycle); both 0 at every index that is no label.  Hooking and pointer jumping as
 *   d3d_mesh_components: the host reads flag (one device int32) once per round and waits on the stream; rounds (host, may be
 *   null) gets the number of hooking launches, which may differ from run to run; the outputs do not. */
int d3d_mesh_boundary_loops(const int* faces, long long n_faces, long long n_vertices, const unsigned char* boundary, const int* out_count,
                            const int* in_count, int* label, int* count, int* bad, int* flag, int* rounds, d3d_stream_t stream);

/* d3d_mesh_holes_plan: every label vertex L of a component that is not bad with 3 <= count <= max_edges walks its cycle from
 *   the half-edge whose tail is L along the successors and sums, in walk order from 0: A += x_a x x_b, N += (p1 - p0) x
 *   (p2 - p0) of the half-edge's owner in that face's corner order, S += x_a.  s [n_vertices] fp64 at L = (A_x N_x + A_y N_y) +
 *   A_z N_z; centroid [n_vertices, 3] fp32 at L = fp32(S / count); position [n_vertices] int32 = the walk position of the
 *   half-edge leaving the vertex (-1: not walked); qualify [n_vertices] int32 at L = 1 when s < 0 (the faces lie outside the
 *   loop: a hole).  s, centroid and qualify are 0 everywhere else.  vertex_offset / face_offset [n_vertices] int32 = the
 *   exclusive scans of qualify and of qualify * count; totals [2] int64 = the new vertices and the new faces.
 *   3 <= max_edges <= D3D_MESH_HOLE_MAX_EDGES. */
int d3d_mesh_holes_plan(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* successor,
                        const int* owner, const int* label, const int* count, const int* bad, int max_edges, void* scratch,
                        size_t scratch_bytes, double* s, float* centroid, int* qualify, int* position, int* vertex_offset, int* face_offset,
                        long long* totals, d3d_stream_t stream);

/* d3d_mesh_holes_emit: out_vertices [n_vertices + n_holes, 3] = vertices, then centroid[L] of every qualifying label L at
 *   n_vertices + vertex_offset[L]; out_faces [n_faces + n_added, 3] = faces, then for every half-edge a->b of such a component
 *   the face (b, a, n_vertices + vertex_offset[L]) at n_faces + face_offset[L] + position[a].  n_holes, n_added: the plan's
 *   totals, read by the host; n_vertices + n_holes and n_faces + n_added stay below 2^31.  The outputs are not the inputs. */
int d3d_mesh_holes_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* successor,
                        const int* label, const int* qualify, const int* position, const int* vertex_offset, const int* face_offset,
                        const float* centroid, long long n_holes, long long n_added, float* out_vertices, int* out_faces,
                        d3d_stream_t stream);

/*
 * DESIGN.md §4.13 -- texturing the surface mesh from the views (the semantics are this project's, deep3d_aerial_amd/texture.py
 * states them in full; they do not claim to match OpenMVS's TextureMesh).  A mesh is vertices [n_vertices, 3] fp32 and faces
 * [n_faces, 3] int32, n_vertices < 2^31, 3 n_faces < 2^31; faces with an index outside 0 .. n_vertices - 1 are skipped (the
 * caller refuses them).  A view is a d3d_ortho_view_t record (ortho's fp64 projection); views and camera tables are DEVICE
 * arrays, and a camera table (rects, texcoords: depth and rgba unused) or a fill's view list is sorted by increasing id.  Every
 * pointer is DEVICE memory except `rounds`.  No float atomics; the integer atomics are min / max.
 */
/* Scratch of d3d_texture_select and d3d_texture_charts (the larger of the two; 0 for an out-of-range argument). */
size_t d3d_texture_scratch_bytes(long long n_faces, int n_views);

/* d3d_texture_select: MIN-MERGES the keys of n_views views into key [n_faces] int64 (INT64_MAX before the first call).  Per
 *   face, in fp64 without contraction: corners a, b, c; nrm = (b - a) x (c - a), g = ((a + b) + c) / 3; a face with nrm = 0 gets
 *   nothing.  A view is a candidate when every corner has p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1; nrm . (C - g) > 0; the
 *   depth D at (floor(v(g) + 0.5), floor(u(g) + 0.5)) is finite and > 0; p2(g) <= D (1 + depth_tolerance).  A =
 *   0.5 |(ub - ua)(vc - va) - (uc - ua)(vb - va)|, s = 1 / A (rejected when A = 0 or s is not finite), key = (bits(fp32(s)) << 32)
 *   | id.  A per-block cull over the box of 256 faces only skips work. */
int d3d_texture_select(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const d3d_ortho_view_t* views,
                       int n_views, double depth_tolerance, void* scratch, size_t scratch_bytes, long long* key, d3d_stream_t stream);

/* d3d_texture_edges: edge_key [3 n_faces] int64: slot 3 f + k holds the k-th distinct edge {i, j} of face f (the pairs (a,b) (b,c)
 *   (c,a) with unequal ends, each unordered pair once) as min(i,j) * n_vertices + max(i,j) when key[f] is not INT64_MAX, and
 *   INT64_MAX otherwise. */
int d3d_texture_edges(const int* faces, long long n_faces, long long n_vertices, const long long* key, long long* edge_key,
                      d3d_stream_t stream);

/* d3d_texture_charts: edge_sorted / face_sorted [n_pairs]: the (edge key, face) pairs sorted by edge key, and by the winner's id
 *   within equal edge keys.  Faces with a winner join when they share an edge and the winner's id; label [n_faces] int32 gets the
 *   smallest face index of each face's chart (hooking and pointer jumping; the host reads flag, one device int32, once per
 *   round), chart [n_faces] int32 the chart number (roots numbered in increasing label order) or -1 for a face with no winner,
 *   n_charts (one device int64) their count.  rounds (host, may be null) gets the number of hooking launches. */
int d3d_texture_charts(const long long* edge_sorted, const int* face_sorted, long long n_pairs, const long long* key, long long n_faces,
                       void* scratch, size_t scratch_bytes, int* label, int* chart, int* flag, long long* n_charts, int* rounds,
                       d3d_stream_t stream);

/* d3d_texture_rects: rect [n_charts, 4] int32 gets (x0, y0, x1, y1), inclusive: over the corners of the chart's faces projected in
 *   the winner's view (camera table cams, looked up by id), x0 = max(0, floor(min u) - pad), x1 = min(W-1, ceil(max u) + pad), y
 *   alike.  pad >= 1. */
int d3d_texture_rects(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* key,
                      const int* chart, long long n_charts, const d3d_ortho_view_t* cams, int n_cams, int pad, int* rect,
                      d3d_stream_t stream);

/* d3d_texture_fill: table [n_charts, 8] int32 (x0, y0, w, h, ox, oy, page, id), page_row [n_pages + 1] int64 (page k's rows of
 *   the atlas are page_row[k] .. page_row[k+1] - 1), atlas [page_row[n_pages], page_width] RGBA8.  work [n_work, 2] int32 lists
 *   (chart, band): rows 8 band .. 8 band + 7 of the chart's rect.  Texel (ox + dx, oy + dy) of the chart's page gets pixel
 *   (x0 + dx, y0 + dy) of the view of `id` among this call's views; charts of other views are left as they are. */
int d3d_texture_fill(const int* work, long long n_work, const int* table, long long n_charts, const long long* page_row, int n_pages,
                     const d3d_ortho_view_t* views, int n_views, int page_width, unsigned int* atlas, d3d_stream_t stream);

/* d3d_texture_empty: every texel of atlas [n_texels] RGBA8 whose alpha is 0 (no fill wrote it) becomes empty_rgba with alpha 255. */
int d3d_texture_empty(unsigned int* atlas, long long n_texels, unsigned int empty_rgba, d3d_stream_t stream);

/* d3d_texture_texcoords: texcoord [n_faces, 6] fp32 and texnumber [n_faces] int32.  Corner (u, v) in the chart's view:
 *   s = (((u - x0) + ox) + 0.5) / page_width, t = 1 - (((v - y0) + oy) + 0.5) / page_height in fp64, rounded to fp32; texnumber the
 *   page.  A face with no chart gets (1 / page_width, 1 - 1 / height of page 0) at every corner and page 0. */
int d3d_texture_texcoords(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* key,
                          const int* chart, const int* table, long long n_charts, const long long* page_row, int n_pages,
                          const d3d_ortho_view_t* cams, int n_cams, int page_width, float* texcoord, int* texnumber,
                          d3d_stream_t stream);

/*
 * DESIGN.md §4.18 -- levelling the colour seams between the texture's charts (deep3d_aerial_amd/texture.py states the rules in
 * full; they are this project's).  A node is a distinct (chart, vertex) pair over the corners of faces with a chart, its key
 * chart * n_vertices + vertex (int64); nodes [n_nodes] holds the keys in increasing order and a node's number is its index.
 * f, b and g are [n_nodes, 4] fp32 records (R, G, B, 0).  table, page_row, cams and atlas are d3d_texture_fill's.  Every pointer
 * is DEVICE memory except d3d_texture_level_solve's `iterations` and `converged`.  No float atomics; the one integer atomic is
 * the coverage's 64-bit min.
 */
/* Scratch of d3d_texture_level_solve (0 for an out-of-range argument). */
size_t d3d_texture_level_scratch_bytes(long long n_nodes);

/* d3d_texture_level_incidence: incidence [3 n_faces] int64 = the node key of each corner of a face with chart[f] >= 0, INT64_MAX
 *   otherwise; edge_key [3 n_faces] int64 = the distinct edges of EVERY face as min(i,j) * n_vertices + max(i,j) (d3d_texture_edges
 *   lists only faces with a winner), INT64_MAX in unused slots. */
int d3d_texture_level_incidence(const int* faces, long long n_faces, long long n_vertices, const int* chart, long long* incidence,
                                long long* edge_key, d3d_stream_t stream);

/* d3d_texture_level_pairs: face_node [3 n_faces] int32 = the node of each corner (-1: no chart).  edge_sorted / face_sorted
 *   [n_pairs]: the (edge key, face) pairs sorted by edge key.  seam [2 n_pairs] int64: the first pair of a run of exactly two
 *   pairs whose faces have different charts c1 < c2 (both >= 0) writes (node(c1, v) << 32) | node(c2, v) for the edge's two ends
 *   v; every other slot gets INT64_MAX.  smooth [3 n_faces] int64: (min << 32) | max over the distinct edges between the corner
 *   nodes of a face with a chart, INT64_MAX otherwise.  The caller makes each list distinct and sorted. */
int d3d_texture_level_pairs(const int* faces, long long n_faces, long long n_vertices, const int* chart, const long long* nodes,
                            long long n_nodes, const long long* edge_sorted, const int* face_sorted, long long n_pairs, int* face_node,
                            long long* seam, long long* smooth, d3d_stream_t stream);

/* d3d_texture_level_csr: entry [n_entries] int64 = (row << 32) | column, sorted: every seam pair and smoothness edge in both
 *   directions.  row_ptr [n_nodes + 1], column [n_entries] int32, weight [n_entries] fp32 = 1 between nodes of different charts,
 *   `smooth` (lambda >= 0) inside a chart. */
int d3d_texture_level_csr(const long long* entry, long long n_entries, const long long* nodes, long long n_nodes, long long n_vertices,
                          float smooth, int* row_ptr, int* column, float* weight, d3d_stream_t stream);

/* d3d_texture_level_samples: f[node] = the bilinear tap of atlas at x = (u - x0) + ox, y = ((v - y0) + oy) + page_row of the
 *   node's vertex in its chart's view, in fp64 ((w00 c00 + w10 c10) + w01 c01) + w11 c11 per channel, rounded to fp32; the taps
 *   are clamped to the chart's rect.  b[i] = the sum over row i's entries j of another chart, in column order, of f[j] - f[i],
 *   in fp32. */
int d3d_texture_level_samples(const float* vertices, long long n_vertices, const long long* nodes, long long n_nodes, const int* row_ptr,
                              const int* column, long long n_entries, const int* table, long long n_charts, const long long* page_row,
                              int n_pages, const d3d_ortho_view_t* cams, int n_cams, int page_width, const unsigned int* atlas, float* f,
                              float* b, d3d_stream_t stream);

/* d3d_texture_level_solve: conjugate gradients for (L + anchor I) g = b from g = 0, per channel, on fp32 vectors with fp64 dot
 *   products folded from fixed slots in slot order (the same bits on every run).  A channel stops, and is frozen, once
 *   r . r <= tolerance^2 b . b; the solve stops when every channel has, or after max_iterations.  The host reads the state once
 *   per 16 iterations.  iterations, converged: HOST ints.  scratch: d3d_texture_level_scratch_bytes(n_nodes) bytes. */
int d3d_texture_level_solve(const int* row_ptr, const int* column, const float* weight, long long n_entries, const float* b,
                            long long n_nodes, float anchor, double tolerance, int max_iterations, void* scratch, size_t scratch_bytes,
                            float* g, int* iterations, int* converged, d3d_stream_t stream);

/* d3d_texture_level_cover: MIN-MERGES into cover [atlas rows, page_width] int64 (INT64_MAX before) the key
 *   (bits(fp32(d2)) << 32) | face of every face with a chart at every texel of its chart's rect whose centre lies within d2 <= 2
 *   of the face's projected triangle (fp64, texel coordinates X = (u - x0) + ox, Y = (v - y0) + oy; d2 = 0 inside). */
int d3d_texture_level_cover(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* chart,
                            const int* table, long long n_charts, const long long* page_row, int n_pages, const d3d_ortho_view_t* cams,
                            int n_cams, int page_width, long long* cover, d3d_stream_t stream);

/* d3d_texture_level_apply: work [n_work, 2] int32 lists (chart, band) as d3d_texture_fill's.  A covered texel's channels become
 *   clamp(rint(colour + ((w0 g0 + w1 g1) + w2 g2)), 0, 255) in fp32, w the barycentric weights (fp64, rounded to fp32) of the
 *   closest point of the covering face, g0 .. g2 its corner nodes' g; alpha is unchanged. */
int d3d_texture_level_apply(const int* work, long long n_work, const float* vertices, long long n_vertices, const int* faces,
                            long long n_faces, const int* chart, const int* face_node, const float* g, long long n_nodes, const int* table,
                            long long n_charts, const long long* page_row, int n_pages, const d3d_ortho_view_t* cams, int n_cams,
                            int page_width, const long long* cover, unsigned int* atlas, d3d_stream_t stream);

/*
 * DESIGN.md §4.22 -- levelling the texture's seams locally: an integer relaxation over the texels within `radius` of a seam, every
 * chart an independent problem (deep3d_aerial_amd/texture.py states the rules in full; they are this project's).  Corrections are
 * integers in units of 1/64 grey level.  state [atlas rows, page_width] int64, one word per texel: the corrections of R, G and B
 * as int16 in bits 0 .. 15, 16 .. 31 and 32 .. 47, the distance from the seam texels in bits 48 .. 55 (255: not reached), bit 56
 * "in the domain" (a face of the rect's chart covers the texel), bit 57 "seam texel".  table, page_row, cams and atlas are
 * d3d_texture_fill's, cover is d3d_texture_level_cover's, work [n_work, 2] int32 lists (chart, band of 8 rows) as
 * d3d_texture_fill's.  Every pointer is DEVICE memory except d3d_texture_local_sweeps' `sweeps_run`.  No float atomics; the one
 * integer atomic counts a sweep's changed texels.  radius is 1 .. 254.
 */
/* The words of state that fit into the LDS of a CU: 160 KiB / 8. */
long long d3d_texture_local_lds_words(void);

/* d3d_texture_local_seams: edge_sorted / face_sorted [n_pairs] are d3d_texture_level_pairs'.  seam [n_pairs, 4] int32: the first
 *   pair of a run of exactly two pairs whose faces have different charts (both >= 0) writes (a, b, c1, c2), a < b the edge's ends
 *   and c1 < c2 the charts; every other row gets -1. */
int d3d_texture_local_seams(const long long* edge_sorted, const int* face_sorted, long long n_pairs, const int* chart, long long n_faces,
                            long long n_vertices, int* seam, d3d_stream_t stream);

/* d3d_texture_local_count: seams [n_seams, 4] int32 (a, b, c1, c2).  count[i] = S = ceil(max(L_c1, L_c2)) + 1 with
 *   L_c = max(|Xb - Xa|, |Yb - Ya|) of the ends in chart c's atlas coordinates (d3d_texture_level_samples' x and y, fp64); 0 for an
 *   edge that is skipped (a bad record or chart, a missing view, an end that does not project). */
int d3d_texture_local_count(const float* vertices, long long n_vertices, const int* seams, long long n_seams, const int* table,
                            long long n_charts, const long long* page_row, int n_pages, const d3d_ortho_view_t* cams, int n_cams,
                            int page_width, int* count, d3d_stream_t stream);

/* d3d_texture_local_samples: scan [n_seams + 1] int64 is the exclusive scan of the counts, n_samples its last entry.  Sample k of
 *   edge i lies at t = k / (S - 1) (0 when S = 1), P = Pa + t (Pb - Pa) per chart; its colour in a chart is
 *   d3d_texture_level_samples' tap, not rounded; e = floor(32 (colour_c2 - colour_c1) + 0.5) per channel.  Sample j = scan[i] + k
 *   writes texel[2 j] = the index (row * page_width + column) of chart c1's texel (floor(X + 0.5), floor(Y + 0.5)), kept inside
 *   the rect, with rec[2 j] = +e (3 int32), and texel[2 j + 1], rec[2 j + 1] = chart c2's texel with -e.  texel [2 n_samples]
 *   int64, rec [2 n_samples, 3] int32. */
int d3d_texture_local_samples(const float* vertices, long long n_vertices, const int* seams, long long n_seams, const long long* scan,
                              long long n_samples, const int* table, long long n_charts, const long long* page_row, int n_pages,
                              const d3d_ortho_view_t* cams, int n_cams, int page_width, const unsigned int* atlas, long long* texel,
                              int* rec, d3d_stream_t stream);

/* d3d_texture_local_fold: WRITES state [n_texels]: "in the domain" where cover is not INT64_MAX, distance 255, corrections 0; then
 *   texel / rec [n_records] sorted by texel: a run of n records of sum s (int64) makes its texel a seam texel of distance 0 with
 *   D = (2 s + n) // (2 n) per channel (floor division).  A texel outside 0 .. n_texels - 1 or outside the domain is skipped. */
int d3d_texture_local_fold(const long long* texel, const int* rec, long long n_records, const long long* cover, long long n_texels,
                           long long* state, d3d_stream_t stream);

/* d3d_texture_local_band: the distances of the work items' texels: 0 on seam texels; round r = 1 .. radius gives r to every domain
 *   texel not yet reached that has a 4-neighbour of distance r - 1 inside its chart's rect and domain; 255 elsewhere. */
int d3d_texture_local_band(const int* work, long long n_work, const int* table, long long n_charts, const long long* page_row, int n_pages,
                           int page_width, long long* state, int radius, d3d_stream_t stream);

/* d3d_texture_local_sweeps: at most `iterations` (1 .. 65535) sweeps over the work items' texels.  A sweep updates the active
 *   texels (distance 1 .. radius) with (column + row) even, then those with it odd, in place: c = (2 s + n) // (2 n) per channel,
 *   s the sum and n the count of the 4-neighbours inside the rect and the domain.  changed [iterations] int32 (device): the
 *   texels each sweep changed; the host reads them once per 16 sweeps and stops after the first sweep that changed nothing.
 *   sweeps_run: HOST int, the sweeps that changed something. */
int d3d_texture_local_sweeps(const int* work, long long n_work, const int* table, long long n_charts, const long long* page_row,
                             int n_pages, int page_width, long long* state, int radius, int iterations, int* changed, int* sweeps_run,
                             d3d_stream_t stream);

/* d3d_texture_local_chart: the same distances and sweeps with one workgroup per chart of list [n_list] int32, the chart's rect held
 *   in LDS: every listed rect must satisfy ((h + 2) (w + 1) + 4) * 8 <= lds_bytes <= 160 KiB (a larger one is left as it is).
 *   iterations 0 .. 65535, 0: the distances only.  sweeps [n_charts] int32: per listed chart the sweeps that changed something. */
int d3d_texture_local_chart(const int* list, long long n_list, const int* table, long long n_charts, const long long* page_row, int n_pages,
                            int page_width, long long* state, int radius, int iterations, int lds_bytes, int* sweeps, d3d_stream_t stream);

/* d3d_texture_local_apply: every domain texel of distance <= radius gets channel = clamp(channel + ((c + 32) >> 6), 0, 255); alpha
 *   is unchanged. */
int d3d_texture_local_apply(const int* work, long long n_work, const int* table, long long n_charts, const long long* page_row,
                            int n_pages, int page_width, const long long* state, int radius, unsigned int* atlas, d3d_stream_t stream);

/*
 * DESIGN.md §4.19 -- smoothing the texture's view choice over the mesh (deep3d_aerial_amd/texture.py states the rule in full; it
 * is this project's).  A candidate list is cand [n_faces, K] int64, K = d3d_texture_candidates_max(): per face the K smallest
 * keys of d3d_texture_select's format that its tests accept, increasing, padded with INT64_MAX.  Every pointer is DEVICE memory
 * except d3d_texture_smooth's `rounds_run`.  No float atomics; the one integer atomic counts a round's commits.
 */
/* K = 16. */
int d3d_texture_candidates_max(void);

/* d3d_texture_candidates: MERGES the keys of n_views views into cand (every entry INT64_MAX before the first call): the K
 *   smallest of the list and the new keys, a key the list already holds counted once.  The cull, the per-view tests and the key
 *   are d3d_texture_select's, so cand[f][0] over all views is its key[f].  scratch: d3d_texture_scratch_bytes(n_faces, n_views). */
int d3d_texture_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const d3d_ortho_view_t* views,
                           int n_views, double depth_tolerance, void* scratch, size_t scratch_bytes, long long* cand, d3d_stream_t stream);

/* d3d_texture_candidates_merge: out = per face the K smallest distinct keys of the lists a and b; out may be a or b. */
int d3d_texture_candidates_merge(const long long* a, const long long* b, long long n_faces, long long* out, d3d_stream_t stream);

/* Scratch of d3d_texture_smooth (0 for an out-of-range size). */
size_t d3d_texture_smooth_scratch_bytes(long long n_faces);

/* d3d_texture_smooth: face_offset / face_index are d3d_mesh_decimate_incidence's outputs for the same mesh (its size limit
 *   holds: 6 n_faces < 2^31).  A face has a winner when its three indices are distinct and in range and cand[f][0] is not
 *   INT64_MAX; view ids (the keys' low words) are 0 .. 2^31 - 2.  With s_k = fp32 from (cand[f][k] >> 32), d_k = 1 - s_0 / s_k;
 *   candidate k is admissible when k = 0 or it is a key and d_k <= max_loss.  Two faces with winners are neighbours with weight
 *   w = the number of vertices they share.  From label 0, per round: n_k = the weighted count of neighbours whose current id
 *   differs from candidate k's, c_k = d_k + weight * float(n_k) (fp32, each operation rounded), best = the admissible k of
 *   smallest (c_k, k), gain = c_label - c_best; a face with gain > 0 has priority (bits(gain) << 32) | (2^32 - 1 - f) and takes
 *   best when its priority exceeds every neighbour's.  commits [rounds] int32 gets each round's number of changes; the host
 *   reads it once per 8 rounds and stops after the first round without a change, or after `rounds` (1 .. 1024) rounds;
 *   rounds_run (HOST, may be null) gets the rounds up to and including that one.  label [n_faces] int32 = the chosen candidate
 *   (-1 without a winner), key_out [n_faces] int64 = cand[f][label[f]] (INT64_MAX without a winner).  weight > 0,
 *   0 <= max_loss <= 1. */
int d3d_texture_smooth(const long long* cand, long long n_faces, const int* faces, long long n_vertices, const int* face_offset,
                       const int* face_index, float weight, float max_loss, int rounds, void* scratch, size_t scratch_bytes, int* label,
                       long long* key_out, int* commits, int* rounds_run, d3d_stream_t stream);

/*
 * DESIGN.md §4.20 -- rejecting photo-inconsistent views from the candidate lists (deep3d_aerial_amd/texture.py states the rule in
 * full; it is this project's).  col [n_faces, K] int32 holds one colour word per slot of cand, 0 = "no colour".  Every pointer is
 * DEVICE memory.  No float atomics; the one integer atomic adds a wave's share of the four counters.
 */
/* d3d_texture_face_colors: the colour of every face in every candidate view of this call's table.  For slot k of face f whose
 *   key is not INT64_MAX, whose id (the key's low word) is in `views` (sorted by id) with a non-null rgba, whose indices are in
 *   range and whose three corners project in front of the view with finite (u, v) (fp64, no contraction, as
 *   d3d_texture_texcoords): four samples in image space, s0 = ((p0 + p1) + p2) / 3 and s_{i+1} = ((4 p_i + p_j) + p_k) / 6 with
 *   j < k the other two corners; each is d3d_ortho_colorize's bilinear tap (x0 = floor(u), fx = u - x0, taps clamped to the image,
 *   ((w00 c00 + w10 c10) + w01 c01) + w11 c11 in fp64, not rounded); per channel q = clamp(floor((((t0 + t1) + t2) + t3) + 0.5),
 *   0, 1020), four times the mean in quarter grey levels; col[f][k] = 2^30 | qR << 20 | qG << 10 | qB.  Every other slot is left as
 *   it was, so calls over disjoint sets of views accumulate into one col (all 0 before the first). */
int d3d_texture_face_colors(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* cand,
                            const d3d_ortho_view_t* views, int n_views, int* col, d3d_stream_t stream);

/* d3d_texture_outliers: the vote, all integer.  A slot is valid when its key is not INT64_MAX and its col is not 0; n = the
 *   number of valid slots; a face with n < 3 is left alone.  Per channel med = the lower median, the value of rank (n - 1) >> 1
 *   among the valid values in increasing order; dev_k = max over the channels of |q_k - med|; slot k is an outlier when dev_k > T
 *   (0 .. 1020).  When every valid slot is an outlier the face keeps its list (kept_all).  cand_out [n_faces, K] gets the keys
 *   that are left, in their order, padded with INT64_MAX; it may be cand.  rejected [n_faces] int32: bit k set when slot k was
 *   removed.  counts [4] int32 (cleared here): faces with n >= 3, faces whose column 0 changed, slots removed, kept_all faces. */
int d3d_texture_outliers(const long long* cand, const int* col, long long n_faces, int T, long long* cand_out, int* rejected, int* counts,
                         d3d_stream_t stream);

/*
 * DESIGN.md §4.21 -- refining the surface mesh against the images: a plane sweep per vertex along its normal and a screened
 * smoothing of the displacement (deep3d_aerial_amd/refine.py states the rule in full; it is this project's and does not claim to
 * match OpenMVS's RefineMesh).  Vertices move, nothing else: topology, face order and vertex count stay.  A mesh is vertices
 * [n_vertices, 3] fp32 and faces [n_faces, 3] int32, 0 < n_vertices < 2^31, 6 n_faces < 2^31; a view is a d3d_ortho_view_t record.
 * Every pointer is DEVICE memory.  The geometry is fp64 without contraction, sums left to right; no float atomics; the one integer
 * atomic adds a wave's share of the four counters.  n_vertices = 0 is an argument error: nothing is launched.
 */
/* RV = 4: the keys per vertex of the view lists. */
int d3d_mesh_refine_views_max(void);

/* d3d_mesh_refine_frames: face_offset / face_index are d3d_mesh_decimate_incidence's outputs and fixed d3d_mesh_adjacency's for the
 *   same mesh.  N = the sum over the vertex's row, in row order, of (b - a) x (c - a) of the faces whose three indices are in
 *   range and distinct (a, b, c the face's corners in its own order); L = sqrt((Nx^2 + Ny^2) + Nz^2).  A vertex is active when it
 *   has such a face, is not fixed, and N and L are finite with L > 0.  frame [n_vertices, 9] fp64 = (n, t1, t2): n = N / L;
 *   j = the axis of smallest |n_j|, ties to the lowest; c = e_j x n = (0, -nz, ny) | (nz, 0, -nx) | (-ny, nx, 0), t1 = c /
 *   sqrt((cx^2 + cy^2) + cz^2); t2 = n x t1.  All nine are 0 for an inactive vertex.  active [n_vertices] uint8. */
int d3d_mesh_refine_frames(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* face_offset,
                           const int* face_index, const unsigned char* fixed, double* frame, unsigned char* active, d3d_stream_t stream);

/* d3d_mesh_refine_views: MERGES the keys of n_views views into list [n_vertices, RV] int64 (every entry INT64_MAX before the first
 *   call): per active vertex the RV smallest distinct keys, increasing, padded with INT64_MAX, so the list does not depend on the
 *   order or the batching of the views.  View V (with a depth map) sees vertex X when p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1
 *   (d3d_ortho_select's projection), dot = (nx dx + ny dy) + nz dz > 0 with d = C - X, the depth D at pixel (floor(v + 0.5),
 *   floor(u + 0.5)) is finite and > 0, and p2 <= D (1 + depth_tolerance) + reach * step.  s = 1 - dot / sqrt((dx^2 + dy^2) + dz^2),
 *   finite; key = (bits(fp32(s)) << 32) | id.  An inactive vertex's row is left as it is.  reach 1 .. 7, step > 0. */
int d3d_mesh_refine_views(const float* vertices, long long n_vertices, const double* frame, const unsigned char* active,
                          const d3d_ortho_view_t* views, int n_views, double depth_tolerance, int reach, double step, long long* list,
                          d3d_stream_t stream);

/* d3d_mesh_refine_match: the sweep and the pick.  `views` is sorted by id; a slot of the list is present when its key is not
 *   INT64_MAX and its id is in `views` with a non-null rgba.  A vertex that is inactive or has fewer than two keys gets kstar -1,
 *   weight 0, d0 0.  Hypothesis k = 0 .. 2 reach: X_k = X + ((k - reach) step) n.  Patch: the 25 points (X_k + (a spacing) t1) +
 *   (b spacing) t2, a, b = -2 .. 2, b-major; a point is valid in a view when p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1; its
 *   grey q = clamp(floor(4 ((tR + tG) + tB) + 0.5), 0, 3060), t = d3d_ortho_colorize's bilinear tap, unrounded.  Pair j = 1 .. 3 is
 *   (slot 0, slot j), both present; with int64 sums over the patch, num = 25 S(ab) - S(a) S(b), va = 25 S(aa) - S(a)^2, vb alike;
 *   the pair is valid at k when all 25 points are valid in both views and va, vb >= min_variance (>= 1); z = (double)num /
 *   sqrt((double)va (double)vb).  A pair is used when it is valid at every k; score_k = (the sum of z over the used pairs, in pair
 *   order) / their number; without a used pair: kstar -1, weight 0, d0 0.  kstar = the k of largest score, ties to the smaller
 *   |k - reach|, then the smaller k; weight = score < min_score ? 0 : 1; when 0 < kstar < 2 reach and den = (s- - 2 s0) + s+ < 0,
 *   delta = clamp(0.5 (s- - s+) / den, -0.5, 0.5), else 0; d0 = fp32(((kstar - reach) + delta) step).  kstar [n_vertices] int32,
 *   weight and d0 [n_vertices] fp32.  counts [4] int32 (cleared here): active vertices, vertices with two keys or more, vertices
 *   with a used pair, vertices with weight 1. */
int d3d_mesh_refine_match(const float* vertices, long long n_vertices, const double* frame, const unsigned char* active,
                          const long long* list, const d3d_ortho_view_t* views, int n_views, int reach, double step, double spacing,
                          long long min_variance, double min_score, int* kstar, float* weight, float* d0, int* counts,
                          d3d_stream_t stream);

/* d3d_mesh_refine_relax: the screened smoothing of the displacement over the CSR of d3d_mesh_adjacency, fp32, every operation
 *   rounded.  d = weight * d0 at first; then `iterations` Jacobi steps d <- (weight * d0 + lambda * m) / (weight + lambda), m =
 *   (the sum of the neighbours' d in CSR order, from 0) / fp32(their number).  An inactive vertex holds 0 and counts as a
 *   neighbour.  out [n_vertices] fp32 gets the result, work [n_vertices] is the other buffer.  lambda > 0, iterations >= 0. */
int d3d_mesh_refine_relax(const float* weight, const float* d0, const unsigned char* active, const long long* offset, const int* nbr,
                          long long n_vertices, float lambda, int iterations, float* work, float* out, d3d_stream_t stream);

/* d3d_mesh_refine_apply: out[v] = fp32(X + (double)d[v] * n) per component for an active vertex, X for any other.  out may be
 *   vertices. */
int d3d_mesh_refine_apply(const float* vertices, long long n_vertices, const double* frame, const unsigned char* active, const float* d,
                          float* out, d3d_stream_t stream);

/*
 * DESIGN.md §4.23 -- subdividing the surface mesh where the images outresolve it: every edge whose projection is longer than
 * max_edge pixels in some view that sees both its ends is split at its midpoint, with conforming face splits (the rule is this
 * project's, deep3d_aerial_amd/subdivide.py states it in full; it does not claim to match OpenMVS's RefineMesh subdivision).  A
 * mesh is vertices [n_vertices, 3] fp32 and faces [n_faces, 3] int32, n_vertices < 2^31, 6 n_faces < 2^31; a face with an index
 * outside 0 .. n_vertices - 1 or with a repeated index comes through unsplit (the caller refuses such a mesh).  edges [max_edges,
 * 2] int32 and *n_edges (device int64) are d3d_mesh_decimate_edges' outputs for the same mesh: the undirected edges a < b in
 * (a, b) lexicographic order; the passes read min(*n_edges, max_edges) of them.  A view is a d3d_mesh_view_t record (its
 * confidence map is not read).  Every pointer is DEVICE memory.  All arithmetic is fp64 without contraction, rounded to fp32
 * only where said; no atomics of any kind.
 */
/* d3d_mesh_subdivide_measure: MAX-MERGES into measure [max_edges] fp64 (all 0 before the first call).  View V sees an endpoint X
 *   under d3d_ortho_select's candidate test: p = R X + t, q = K p, each row summed left to right, p2 > 0, q2 > 0, u = q0 / q2,
 *   v = q1 / q2, 0 <= u <= W-1, 0 <= v <= H-1, the depth D at pixel (floor(v + 0.5), floor(u + 0.5)) is finite and > 0, and
 *   p2 <= D * (1 + depth_tolerance).  A view that sees both ends of edge e contributes l2 = (ua - ub)^2 + (va - vb)^2; a
 *   non-finite l2 rejects it.  measure[e] = max(measure[e], the largest l2): it does not depend on the order, the batching or
 *   the split of the views.  Entries from *n_edges on are left as they are.  depth_tolerance finite, >= 0; n_views < 2^20. */
int d3d_mesh_subdivide_measure(const float* vertices, long long n_vertices, const int* edges, const long long* n_edges, long long max_edges,
                               const d3d_mesh_view_t* views, int n_views, double depth_tolerance, double* measure, d3d_stream_t stream);

/* Scratch of d3d_mesh_subdivide_plan (0 for out-of-range sizes). */
size_t d3d_mesh_subdivide_scratch_bytes(long long n_faces, long long max_edges);

/* d3d_mesh_subdivide_plan: midpoint [max_edges, 3] fp32 = fp32((fp64(x_a) + fp64(x_b)) * 0.5) per component; mark [max_edges]
 *   int32 = 1 when measure[e] > max_edge^2 and the midpoint differs from both ends (in some component); both 0 from *n_edges on.
 *   rank [max_edges] int32 = the exclusive scan of mark: a split edge's new vertex is n_vertices + rank[e].  face_edge [n_faces,
 *   3] int32 = the list index of edge (v_i, v_{i+1}) of face (v0, v1, v2), by binary search of (min, max); all three -1 for a
 *   face that comes through unsplit.  child_count [n_faces] int32 = 1 + the marked edges of the face, child_offset its exclusive
 *   scan.  totals [2] int64 = the split edges and the faces after the split.  max_edge finite, >= 1 (pixels). */
int d3d_mesh_subdivide_plan(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* edges,
                            const long long* n_edges, long long max_edges, const double* measure, double max_edge, void* scratch,
                            size_t scratch_bytes, int* mark, int* rank, float* midpoint, int* face_edge, int* child_count, int* child_offset,
                            long long* totals, d3d_stream_t stream);

/* d3d_mesh_subdivide_emit: out_vertices [n_vertices + n_split, 3] = vertices, then midpoint[e] of every split edge at n_vertices
 *   + rank[e].  out_faces [n_faces_out, 3]: the children of face f from child_offset[f] on, with m_i the new vertex of e_i =
 *   (v_i, v_{i+1}) and the winding kept.  No edge split: (v0, v1, v2).  Only e_i split, (a, b, c) = (v_i, v_{i+1}, v_{i+2}):
 *   (a, m_i, c), (m_i, b, c).  Only e_i unsplit, (a, b, c) alike, p = m_{i+1}, q = m_{i+2}: (p, c, q), then the quad a, b, p, q
 *   cut by the shorter of a-p and b-q, squared lengths (dx^2 + dy^2) + dz^2 in fp64 on the fp32 positions, a tie going to the
 *   diagonal that starts at the smaller of the indices a and b: a-p gives (a, b, p), (a, p, q); b-q gives (a, b, q), (b, p, q).
 *   All three split: (v0, m0, m2), (m0, v1, m1), (m2, m1, v2), (m0, m1, m2).  n_split, n_faces_out: the plan's totals, read by
 *   the host; n_vertices + n_split and 6 n_faces_out stay below 2^31.  The outputs are not the inputs. */
int d3d_mesh_subdivide_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* n_edges,
                            long long max_edges, const int* mark, const int* rank, const float* midpoint, const int* face_edge,
                            const int* child_offset, long long n_split, long long n_faces_out, float* out_vertices, int* out_faces,
                            d3d_stream_t stream);

/*
 * DESIGN.md §4.24 -- collapsing the mesh edges shorter than the images resolve: every edge whose measure (§4.23's: the largest
 * squared pixel length over the views that see both its ends) is above 0 and below min_edge^2 is a candidate for an edge collapse,
 * and the decimation's claim, apply and faces passes (§4.14) take the independent ones with every valid candidate eligible
 * (threshold = LLONG_MAX, no select pass).  The rule is this project's, deep3d_aerial_amd/collapse.py states it in full; it does
 * not claim to match OpenMVS's RefineMesh (nEnsureEdgeSize).  The mesh, offset / nbr / fixed (d3d_mesh_adjacency), face_offset /
 * face_index (d3d_mesh_decimate_incidence), edges and *n_edges (d3d_mesh_decimate_edges) are as §4.14 takes them, measure
 * [max_edges] fp64 is d3d_mesh_subdivide_measure's.  Every pointer is DEVICE memory.  All arithmetic is fp64 without contraction,
 * rounded to fp32 only where said; no atomics.
 */
/* d3d_mesh_collapse_candidates: per edge e = (a, b), a < b, of the first min(*n_edges, max_edges): key [max_edges] int64 and
 *   target [max_edges, 3] fp32.  The edge is short when 0 < measure[e] < min_edge^2.  A fixed end survives and the target t is its
 *   position; with both ends free a survives at t = fp32((fp64(x_a) + fp64(x_b)) * 0.5) per component.  The candidate is valid
 *   when (1) the rows of a and b in nbr share exactly two vertices, (2) |N(a)| + |N(b)| - 4 >= 3, (3) no face at a or b that does
 *   not hold both ends turns over or loses its area with the end at t (old normal . new normal > 0, the normal (p1 - p0) x
 *   (p2 - p0), as d3d_mesh_decimate_candidates judges it), and (4) with L2 = (dx dx + dy dy) + dz dz of x_b - x_a and s =
 *   measure[e] / L2, every w in N(a) or N(b) other than a and b has ((tx - wx)^2 + (ty - wy)^2) + (tz - wz)^2, times s, <=
 *   max_edge^2 (a NaN fails).  key = (bits(fp32(measure[e])) << 32) | (e * 2654435761 mod 2^32) for a short edge with a free end
 *   that is valid, else -1 (also from *n_edges on); target is 0 wherever the key is -1.  min_edge finite, > 0; max_edge finite,
 *   >= 2 min_edge (pixels). */
int d3d_mesh_collapse_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                 const long long* offset, const int* nbr, const unsigned char* fixed, const int* face_offset,
                                 const int* face_index, const int* edges, const long long* n_edges, long long max_edges,
                                 const double* measure, double min_edge, double max_edge, float* target, long long* key,
                                 d3d_stream_t stream);

/*
 * DESIGN.md §4.25 -- flipping the mesh edges whose flip removes a cap triangle: an interior manifold edge (a, b) with the
 * opposite corners c and d is swapped for (c, d) when that raises the worse of the two triangles' shape quality, under a
 * planarity guard, in rounds of independent flips.  Vertices never move, the vertex and face counts never change, the boundary
 * never changes.  The rule is this project's, deep3d_aerial_amd/flip.py states it in full; it does not claim to match OpenMVS's
 * bRemoveSpikes (VCG's RemoveTVertexByFlip).  The mesh (every face three distinct indices in range), offset / nbr
 * (d3d_mesh_adjacency), face_offset / face_index (d3d_mesh_decimate_incidence), edges and *n_edges (d3d_mesh_decimate_edges) are
 * as §4.14 takes them.  Every pointer is DEVICE memory.  All arithmetic is fp64 without contraction, dot products and squared
 * lengths summed left to right, (x x + y y) + z z; integer atomics only.
 */
/* d3d_mesh_flip_candidates: per edge e = (a, b), a < b, of the first min(*n_edges, max_edges): key [max_edges] int64 and opp
 *   [max_edges, 4] int32 = (c, d, f_ab, f_ba).  The edge is a candidate when (3) exactly two faces of a's row hold b, one with
 *   the directed edge a->b (f_ab, its third corner c) and one with b->a (f_ba, its third corner d), and c != d; (4.1) d is not in
 *   c's row of nbr; (4.2) the rows of a and b in nbr each hold more than 3 vertices; (4.3) with n1 = (x_b - x_a) x (x_c - x_a) and
 *   n2 = (x_a - x_b) x (x_d - x_b), n1.n2 >= 0 and (n1.n2)^2 >= cos2_max_angle (|n1|^2 |n2|^2) (a NaN fails); (4.4) the normals of
 *   the new faces (a, d, c) and (b, c, d), taken from their first corner, each have a dot product > 0 with n1 + n2; (5) with
 *   Q = |n|^2 / S^2 of a triangle (n its normal, S = (|p1 - p0|^2 + |p2 - p1|^2) + |p0 - p2|^2, the corners in increasing index
 *   order, Q = 0 when S = 0), min(Q(adc), Q(bcd)) > min(Q(abc), Q(bad)).  key = (bits(fp32(min(Q(abc), Q(bad)))) << 32) |
 *   (e * 2654435761 mod 2^32) for a candidate, else -1 (also from *n_edges on); opp is 0 wherever the key is -1.
 *   cos2_max_angle in [0, 1): the squared cosine of the largest angle between n1 and n2, computed by the caller.  No atomics. */
int d3d_mesh_flip_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                             const long long* offset, const int* nbr, const int* face_offset, const int* face_index,
                             const int* edges, const long long* n_edges, long long max_edges, double cos2_max_angle,
                             long long* key, int* opp, d3d_stream_t stream);

/* d3d_mesh_flip_claim: claim [n_vertices] int64 = the smallest key of the candidates that hold the vertex as a, b, c or d
 *   (64-bit atomicMin), LLONG_MAX where none does; *n_winners = 0. */
int d3d_mesh_flip_claim(long long n_vertices, const int* edges, const long long* key, const int* opp, const long long* n_edges,
                        long long max_edges, long long* claim, long long* n_winners, d3d_stream_t stream);

/* d3d_mesh_flip_apply: out_faces [n_faces, 3] = faces, then every winner (a candidate whose key is the claim of its a, b, c and
 *   d; winners share no vertex, hence no face) writes (a, d, c) to slot f_ab and (b, c, d) to slot f_ba.  win [max_edges] uint8:
 *   1 for a winner; *n_winners gets their number added (d3d_mesh_flip_claim zeroed it).  out_faces is not faces. */
int d3d_mesh_flip_apply(const int* faces, long long n_faces, const int* edges, const long long* key, const int* opp,
                        const long long* n_edges, long long max_edges, const long long* claim, int* out_faces, unsigned char* win,
                        long long* n_winners, d3d_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * View selection from a sparse model (deep3d_aerial_amd/view_selection.py states the rule).
 *
 * The model in dense indices, device memory: image k = 0 .. n_img - 1, point p = 0 .. n_pts - 1; the observations as CSR by image
 * (img_offset [n_img + 1] int64, obs_point [n_obs] int32, -1 = no point); the tracks as CSR by point (trk_offset [n_pts + 1]
 * int64, trk_image [n_trk] int32); xyz [n_pts, 3] fp64; centers [n_img, 3] fp64.  An index outside its range is skipped.
 *
 *   d3d_view_select_lds_images: the counters a workgroup's LDS holds.  A call with rows * n_img <= lds_images (rows = 1 in points
 *     mode, 2 in angle mode; lds_images at most this value) keeps its rows in LDS, any other call in scratch; same bits.
 *   d3d_view_select_scratch_bytes(n_ref, n_img, mode, lds_images): 256 on the LDS path, else min(n_ref, 1024) rows * n_img * 4
 *     bytes rounded up to 256: the rows of one batch of reference images.  0 for arguments the call would refuse.
 *   d3d_view_select_blocks: mask [n_blocks, n_img] uint8, cleared by the call, then mask[b][k] = 1 iff a point p >= p_first whose
 *     track holds k has blocks[b][0] < x < blocks[b][1] and blocks[b][2] < y < blocks[b][3] (blocks [n_blocks, 4] fp64 in device
 *     memory; strict, z untested).  The points before p_first (ids <= 0) are ignored.  At most D3D_VIEW_SELECT_MAX_BLOCKS blocks.
 *   d3d_view_select_rows: for i < n_ref and r = refs[i], over the observations o of r with a point p and the entries s of
 *     track(p): C[s] += 1, and in angle mode (mode 1) S[s] += weight[bin] for s != r, with a = centers[r] - xyz[p],
 *     b = centers[s] - xyz[p], c = ((a_x b_x + a_y b_y) + a_z b_z) / (sqrt(|a|^2) sqrt(|b|^2)) in fp64, every operation rounded
 *     once, weight 0 when a length is 0, and bin the largest k < n_bins with c <= edge[k] (0 when there is none; edge must not
 *     increase).  The score is C in points mode (mode 0) and S in angle mode.  seen[i] = the s != r with C[s] > 0, maxv[i] = the
 *     largest score over s != r, n_src[i] = the s != r with C[s] > 10 and 10 score[s] > maxv[i]; those s, their scores and their
 *     C go to src / score / count from seg_offset[i] on in ascending s, never past seg_offset[i + 1] (seg_offset [n_ref + 1]
 *     int64, not decreasing, at most n_seg).  The entries of a segment from n_src[i] on are not written.  All sums are uint32: the
 *     caller keeps the sum of the track lengths of an image below 2^22.  Integer atomicAdd only, results unused.
 * Null pointers (where the count is not 0), a count outside 0 .. 2^31 - 1, a misaligned or short buffer, overlapping buffers:
 * D3D_ERR_INVALID_ARG before any launch.
 */
#define D3D_VIEW_SELECT_MAX_BLOCKS 512
int d3d_view_select_lds_images(void);
size_t d3d_view_select_scratch_bytes(long long n_ref, int n_img, int mode, long long lds_images);
int d3d_view_select_blocks(const double* xyz, const long long* trk_offset, const int* trk_image, long long n_pts, long long n_trk,
                           long long p_first, int n_img, const double* blocks, int n_blocks, unsigned char* mask, d3d_stream_t stream);
int d3d_view_select_rows(const long long* img_offset, const int* obs_point, long long n_obs, const long long* trk_offset,
                         const int* trk_image, long long n_pts, long long n_trk, int n_img, const int* refs, long long n_ref, int mode,
                         const double* centers, const double* xyz, const double* edge, const unsigned* weight, int n_bins,
                         long long lds_images, void* scratch, size_t scratch_bytes, const long long* seg_offset, long long n_seg,
                         int* seen, unsigned* maxv, int* n_src, int* src, unsigned* score, unsigned* count, d3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEP3D_PLANESWEEP_H */
