"""Weight packing: every function that turns a parameter into the operand tensor a kernel reads.

Pure tensor -> tensor functions (host-side preparation, once per parameter version): no ctypes, no caches, no dispatch
counters -- those live in _runtime.py (derived_weight, _packed, _packed_fold), the operators that choose a packer in
ops.py.  The docstrings state each kernel's K-index contract; they are the specification the CPU tests check
(tests/test_packing_mfma.py, tests/test_fold_packing.py).
"""
import itertools

import numpy as _np
import torch

from . import _lib


def h16_dtype():
    """torch dtype of the library's 16-bit operand format (d3d_h16_format: "f16" by default, "bf16" in a -DD3D_H16_BF16 build):
    what channel-last "h16" volumes and packed 16-bit weight fragments are made of."""
    return torch.float16 if _lib.h16_format() == "f16" else torch.bfloat16


# ----------------------------------------------------------------------------------------
# shared pieces: the three-way split, the 16x16x32 B fragment, the stride-2 parity table
# ----------------------------------------------------------------------------------------
def _split3_bf16(w):
    """fp32 tensor -> its exact three-way bf16 split (hi, mid, lo as fp32 tensors; hi + mid + lo == w in fp32)."""
    w = w.to(torch.float32)
    hi = w.to(torch.bfloat16).to(torch.float32)
    mid = (w - hi).to(torch.bfloat16).to(torch.float32)
    lo = (w - hi - mid).to(torch.bfloat16).to(torch.float32)
    return hi, mid, lo


def _x3(pack, w):
    """[hi | mid | lo] x `pack`: the operands of a bf16x3 kernel (always bfloat16, whatever the library's 16-bit format)."""
    return torch.stack([pack(part, torch.bfloat16) for part in _split3_bf16(w)]).contiguous()


def _pad_b(rows, kblock=32, ncols=None):
    """fp32 GEMM operand [.., K, Co] -> zero-padded dense B [.., K up to a multiple of kblock, ncols]; ncols defaults to Co up
    to a multiple of 16, and a packer whose kernel reads ONE tile passes 16 (a wider weight then raises here)."""
    K, Co = rows.shape[-2:]
    b = torch.zeros(tuple(rows.shape[:-2]) + ((K + kblock - 1) // kblock * kblock, ncols or (max(Co, 16) + 15) // 16 * 16),
                    dtype=torch.float32, device=rows.device)
    b[..., :K, :Co] = rows
    return b


def _frag16(b, dt=None):
    """Dense fp32 B [.., K, N] (K a multiple of 32, N of 16) -> the B fragments of v_mfma_f32_16x16x32_bf16 / _f16,
    [..][K block][N tile][lane][8] as int16 bits: lane l holds column l & 15, rows 8 * (l >> 4) .. + 7 of its block."""
    n = b.dim() - 2
    nkb, ntn = b.shape[-2] // 32, b.shape[-1] // 16
    b = b.reshape(tuple(b.shape[:n]) + (nkb, 4, 8, ntn, 16))                      # [kb][kgroup][j][ntile][n]
    b = b.permute(tuple(range(n)) + (n, n + 3, n + 1, n + 4, n + 2))            # [kb][ntile][kgroup][n][j]
    return b.reshape(tuple(b.shape[:n]) + (nkb, ntn, 64, 8)).to(dt or h16_dtype()).view(torch.int16).contiguous()


def _kidx(k, p, d):
    """THE stride-2 parity table: the kernel index through which tap d (0 | 1) reaches an output coordinate of parity p along one
    axis of a stride-2, padding-1 transposed convolution; None where the class has no such tap.  k = 3 (output_pad 1): an even
    coordinate uses index 1 (d = 0), an odd one index 2 (d = 0) and 0 (d = 1).  k = 4: output 2i + p reads input i - 1 + p + d
    through index 3 - p - 2d."""
    return 3 - p - 2 * d if k == 4 else {(0, 0): 1, (1, 0): 2, (1, 1): 0}.get((p, d))


def _parity_taps(parities, k=3):
    """The taps of one output parity class (p per dimension, 2-D or 3-D), first dimension major: [(d per dim, kernel index per dim)]."""
    dims = [[(d, _kidx(k, p, d)) for d in (0, 1) if _kidx(k, p, d) is not None] for p in parities]
    return [tuple(zip(*tap)) for tap in itertools.product(*dims)]


def _parity_rows(w, parities, k=3):
    """Transposed-conv weight [Ci,Co,k,..] -> the GEMM rows [(tap, ci), Co] of one parity class, taps as in _parity_taps."""
    return torch.cat([w[(slice(None), slice(None)) + kk] for _, kk in _parity_taps(parities, k)]).to(torch.float32)


# ----------------------------------------------------------------------------------------
# 3-D layers (CostRegNet)
# ----------------------------------------------------------------------------------------
def _pack_c8_bf16(w, dt=None):
    """[8,Ci,3,3,3] -> the B operands of v_mfma_f32_16x16x32_bf16 for d3d_conv3d_k3_c8_h16: [kz][K block][lane][8] bf16
    with K = (ky, kx, ci) padded to a multiple of 32 and the 8 output channels in columns 0..7 of 16 (rest zero);
    lane l holds column l & 15, rows 8 * (l >> 4) .. + 7 of its block.  Returned as int16 bits."""
    Co, Ci = w.shape[0], w.shape[1]
    # w[n, ci, kz, ky, kx] -> b[kz, (ky*3+kx)*Ci + ci, n]
    return _frag16(_pad_b(w.permute(2, 3, 4, 1, 0).reshape(3, 9 * Ci, Co)), dt)


def _pack_c8_bf16x3(w):
    """[Co,Ci,3,3,3] -> the B operands of d3d_conv3d_k3_zs_bf16x3: [hi | mid | lo] x _pack_c8_bf16 (the exact three-way bf16 split)."""
    return _x3(_pack_c8_bf16, w)


def _pack_c8_kzfold_bf16(w, dt=None):
    """nn.Conv3d weight [1,Ci,3,3,3] -> B operands of d3d_conv3d_k3_c1_cl_h16: ONE tile per K block whose columns 0, 1, 2 are
    the k_z = 0, 1, 2 slices (K = (k_y, k_x, c_in), padded to a multiple of 32); [K block][lane][8], lane l = column l & 15,
    K rows 8 * (l >> 4) .. + 7.  int16 bits (bf16)."""
    K = 9 * w.shape[1]
    # [ci, kz, ky, kx] -> [ky, kx, ci, kz] -> rows (ky*3+kx)*Ci + ci, column kz
    return _frag16(_pad_b(w[0].permute(2, 3, 0, 1).reshape(K, 3), ncols=16), dt).reshape(-1, 64, 8)


def _pack_c8_kzfold_bf16x3(w):
    """[1,Ci,3,3,3] -> the B operands of d3d_conv3d_k3_c1_bf16x3: [hi | mid | lo] x _pack_c8_kzfold_bf16."""
    return _x3(_pack_c8_kzfold_bf16, w)


def _pack_co8(w):
    """[8,Ci,3,3,3] -> [Ci][ky][kx][kz][8] fp32 for d3d_conv3d_k3_co8 (vector units: no fragments, the 8 outputs innermost)."""
    return w.permute(1, 3, 4, 2, 0)


def _pack_coT8(w):
    """ConvTranspose3d weight [Ci,8,3,3,3] -> [Ci][kz][ky][kx][8] fp32 for d3d_convtranspose3d_k3s2_co8 (vector units)."""
    return w.permute(0, 2, 3, 4, 1)


def _pack_t2_bf16(w, dt=None):
    """nn.ConvTranspose3d weight [Ci,Co,3,3,3] -> B operands of v_mfma_f32_16x16x32_bf16 for d3d_convtranspose3d_k3s2_zs_h16.
    Output parity class (pz,py,px), in the order pz*4 + py*2 + px: taps (dz,dy,dx), d <= p per dimension, enumerated dz-major;
    an even output coordinate uses kernel index 1 (d = 0), an odd one index 2 (d = 0) and 0 (d = 1).  K = (tap, ci) padded to
    a multiple of 32, output channels padded to a multiple of 16; per class [K block][N tile][lane][8] with lane l holding
    column l & 15 and rows 8 * (l >> 4) .. + 7 of its block.  Returned as int16 bits (bf16)."""
    return torch.cat([_frag16(_pad_b(_parity_rows(w, (p >> 2, (p >> 1) & 1, p & 1))), dt).reshape(-1, 8) for p in range(8)])


def _pack_t2_bf16x3(w):
    """nn.ConvTranspose3d weight [Ci,Co,3,3,3] -> the B operands of d3d_convtranspose3d_k3s2_zs_bf16x3: [hi | mid | lo] x _pack_t2_bf16."""
    return _x3(_pack_t2_bf16, w)


def _pack_t2_fold_bf16(w, dt=None):
    """ConvTranspose3d weight [Ci,8,3,3,3] -> A operands of the x-folded form of d3d_convtranspose3d_k3s2_cl_h16: per output
    parity class (pz,py), K = (taps (dz,dy,dx) with dx in {0,1}, dz-major) x ci, GEMM row r = px * 8 + channel: the even
    column (px = 0) uses kernel column 1 of the dx = 0 taps (its dx = 1 entries are zero), the odd one column 2 (dx = 0)
    and 0 (dx = 1).  [class][K block][lane][8], lane l = row l & 15, K rows 8 * (l >> 4) .. + 7.  int16 bits (bf16).
    (Differs from _pack_t2_bf16: both column parities share one tile, so every (dz,dy) tap carries both dx.)"""
    Ci, Co = w.shape[0], w.shape[1]
    assert Co == 8
    parts = []
    for c in range(4):
        rows = []
        for _, (kz, ky) in _parity_taps((c >> 1, c & 1)):
            for dx in range(2):
                r = torch.zeros((Ci, 16), dtype=torch.float32, device=w.device)
                if dx == 0:
                    r[:, 0:8] = w[:, :, kz, ky, _kidx(3, 0, 0)]
                r[:, 8:16] = w[:, :, kz, ky, _kidx(3, 1, dx)]
                rows.append(r)
        parts.append(_frag16(_pad_b(torch.cat(rows)), dt).reshape(-1, 8))
    return torch.cat(parts)


# ----------------------------------------------------------------------------------------
# 2-D layers (slice regularisers, feature pyramids)
# ----------------------------------------------------------------------------------------
def _pack_z2_bf16(w, dt=None):
    """nn.Conv2d weight [Co,Ci,3,3] -> B operands of v_mfma_f32_16x16x32_bf16 for d3d_conv2d_k3_zs_h16: K = (k_y, k_x, c_in)
    padded to a multiple of 32, output channels to a multiple of 16; [K block][N tile][lane][8], lane l = column l & 15,
    K rows 8 * (l >> 4) .. + 7 of its block.  int16 bits (bf16)."""
    Co, Ci = w.shape[0], w.shape[1]
    K = w.shape[2] * w.shape[3] * Ci                                   # (3 x 3; 5 x 5 for d3d_conv2d_k5s2_zs_bf16x3)
    return _frag16(_pad_b(w.permute(2, 3, 1, 0).reshape(K, Co)), dt)   # [ky, kx, ci, co]


def _pack_z2_bf16x3(w):
    """nn.Conv2d weight [Co,Ci,3,3] -> the B operands of d3d_conv2d_k3_zs_bf16x3: [hi | mid | lo] x _pack_z2_bf16."""
    return _x3(_pack_z2_bf16, w)


def _pack_z2_f32(w):
    """nn.Conv2d weight [Co,Ci,3,3] -> fp32 B operands of v_mfma_f32_16x16x4_f32 for d3d_conv2d_k3_zs_f32: K = (k_y, k_x, c_in)
    in blocks of 4, output channels padded to a multiple of 16; [K block][N tile][lane], lane l = column l & 15, K row l >> 4.
    (Differs from _frag16: fp32, 4 K rows per block, one value per lane.)"""
    Co, Ci = w.shape[0], w.shape[1]
    K = 9 * Ci
    b = _pad_b(w.permute(2, 3, 1, 0).reshape(K, Co), kblock=1)
    ntn = b.shape[1] // 16
    return b.reshape(K // 4, 4, ntn, 16).permute(0, 2, 1, 3).reshape(K // 4, ntn, 64).contiguous()


def _pack_t2d_bf16(w, dt=None):
    """nn.ConvTranspose2d weight [Ci,Co,3,3] -> B operands for d3d_convtranspose2d_k3s2_zs_h16: per output parity class
    (py,px), order py*2 + px, taps (dy,dx) with d <= p per dimension, dy-major; an even output coordinate uses kernel index 1
    (d = 0), an odd one index 2 (d = 0) and 0 (d = 1).  K = (tap, ci) padded to 32, 16 output columns; [K block][lane][8]."""
    return torch.cat([_frag16(_pad_b(_parity_rows(w, (c >> 1, c & 1)), ncols=16), dt).reshape(-1, 8) for c in range(4)])


def _pack_t2d_bf16x3(w):
    """nn.ConvTranspose2d weight [Ci,Co,3,3] -> the B operands of d3d_convtranspose2d_k3s2_zs_bf16x3: [hi | mid | lo] x _pack_t2d_bf16."""
    return _x3(_pack_t2d_bf16, w)


def _pack_t2d_f32(w):
    """_pack_t2d_bf16 in fp32 for d3d_convtranspose2d_k3s2_zs_f32: per parity class, K = (tap, ci) in blocks of 4, [K block][lane]
    with lane l = column l & 15, K row l >> 4.  (Differs from _frag16 as _pack_z2_f32 does.)"""
    return torch.cat([_pad_b(_parity_rows(w, (c >> 1, c & 1)), kblock=1, ncols=16).reshape(-1, 64) for c in range(4)]).contiguous()


def _pack_t2d_k4_bf16(w, dt=None):
    """nn.ConvTranspose2d weight [Ci,Co,4,4] (stride 2, padding 1) -> B operands of the k = 4 transposed tile kernel: per output
    parity class (py,px), order py*2 + px, taps (dy,dx) in {0,1}^2 dy-major; output 2i + p reads input i - 1 + p + d through
    kernel index 3 - p - 2d.  K = (tap, ci), 16 output columns; [K block][lane][8] (bf16 bits)."""
    return torch.cat([_frag16(_pad_b(_parity_rows(w, (c >> 1, c & 1), 4), ncols=16), dt).reshape(-1, 8) for c in range(4)])


def _pack_t2d_k4fold_bf16(w, dt=None):
    """The k = 4 transposed weight [Ci,Co<=8,4,4] with both column parities in one 16-column tile: per row parity py, K =
    (dy in {0,1}, patch column dxx in {0,1,2}, ci); columns 0..7 = even output column (dxx = dx), 8..15 = odd one (dxx = 1 + dx).
    (Differs from _pack_t2d_k4_bf16: the K index is the patch column, shared by the two column parities.)"""
    Ci, Co = w.shape[0], w.shape[1]
    parts = []
    for py in range(2):
        b = torch.zeros((6 * Ci, 16), dtype=torch.float32, device=w.device)
        for dy in range(2):
            for dxx in range(3):
                t = dy * 3 + dxx
                for px in range(2):
                    dx = dxx - px
                    if dx in (0, 1):
                        b[t * Ci:(t + 1) * Ci, px * 8:px * 8 + Co] = w[:, :, _kidx(4, py, dy), _kidx(4, px, dx)]
        parts.append(_frag16(_pad_b(b), dt).reshape(-1, 8))
    return torch.cat(parts)


def _pack_t2d_k4_bf16x3(w):
    """[hi | mid | lo] x the k = 4 packing d3d_convtranspose2d_k4s2_zs_bf16x3 takes: column-folded for C_out <= 8."""
    return _x3(_pack_t2d_k4fold_bf16 if w.shape[1] <= 8 else _pack_t2d_k4_bf16, w)


def upsampled_conv_weight(w3):
    """Conv2d weight [Co,Ci,3,3] (padding 1) -> the ConvTranspose2d weight [Ci,Co,4,4] (stride 2, padding 1) with
    conv_transpose2d(f, .) == conv2d(nearest_x2(f), w3): the three taps of an output pixel along an axis fall on two cells
    of f, and the weights of taps sharing a cell add (kernel index 3: tap 0; 1: taps 1 + 2; 0: tap 2; 2: taps 0 + 1)."""
    w = w3.detach().to(torch.float64)
    rows = torch.stack([w[:, :, 2], w[:, :, 1] + w[:, :, 2], w[:, :, 0] + w[:, :, 1], w[:, :, 0]], 2)          # [Co,Ci,4(ky),3]
    full = torch.stack([rows[..., 2], rows[..., 1] + rows[..., 2], rows[..., 0] + rows[..., 1], rows[..., 0]], 3)   # [Co,Ci,4,4]
    return full.permute(1, 0, 2, 3).to(torch.float32).contiguous()


def _pack_t2flip(w):
    """ConvTranspose2d weight [Ci,Co,3,3] -> the Conv2d weight [Co,Ci,3,3] (flipped kernel) whose stride-1 convolution of the
    zero-stuffed input is the transposed convolution (k 3, s 2, p 1, output_pad 1)."""
    return w.flip(2, 3).transpose(0, 1)


def _pack_c2s(w):
    """nn.Conv2d weight [Co,Ci,3,3] -> [Ci up to a multiple of 8][3][3][Co] fp32 for d3d_conv2d_k3_stream (vector units) and for
    the first layer of d3d_conv2d_k3_pair3_bf16x3."""
    Co, Ci = w.shape[0], w.shape[1]
    wp = w.new_zeros(((Ci + 7) // 8 * 8, 3, 3, Co))
    wp[:Ci] = w.permute(1, 2, 3, 0)
    return wp


def _pack_c11(w):
    """[Co,Ci,1,1] -> [Ci][Co] fp32 for d3d_conv1x1_upskip."""
    return w.reshape(w.shape[0], w.shape[1]).t()


def _pack_k1(w):
    """[Co,Ci,1,1] -> [ceil(Co / 8)][Ci][8]: blocks of 8 output channels, zero-padded (d3d_conv2d_k1_f32)."""
    Co, Ci = w.shape[0], w.shape[1]
    nb = (Co + 7) // 8
    wp = w.new_zeros((nb * 8, Ci))
    wp[:Co] = w.reshape(Co, Ci)
    return wp.reshape(nb, 8, Ci).permute(0, 2, 1).contiguous()


def _round_h16(w):
    """The weights as the matrix cores round them (to the library's 16-bit format and back), for the fused slice heads."""
    return w.to(h16_dtype()).float().contiguous()


# ----------------------------------------------------------------------------------------
# MFMA implicit GEMM (d3d_conv_gemm_f32): packed weights and tap lists
# ----------------------------------------------------------------------------------------
def _mpad(co):
    mt = (co + 15) // 16
    return 16 * (4 if mt == 3 else mt)


def _pack_gemm(weight, transposed):
    """Packed GEMM operands of a k=3 conv weight (_runtime._packed caches them).

    conv  [Co,Ci,(3,)3,3] -> one (wpack [T*Ci, mpad], taps int8 [T,3]) with offsets -1..1.
    convT [Ci,Co,(3,)3,3] -> one entry per output-parity class: (parity zyx, wpack, taps) with
    offsets 0/+1 (even outputs: kernel index 1 at o/2; odd: index 0 at (o+1)/2, index 2 at (o-1)/2).
    """
    w = weight.float()
    if w.dim() == 4:
        w = w.unsqueeze(2)  # [.., 1, 3, 3]: z kernel of size 1
    kz_n = w.shape[2]

    def entry(wp, taps, Co):
        pad = torch.zeros((wp.shape[0], _mpad(Co)), dtype=torch.float32, device=w.device)
        pad[:, :Co] = wp
        return pad.contiguous(), _np.array(taps, _np.int8).tobytes(), len(taps)

    if not transposed:
        Co, Ci = w.shape[0], w.shape[1]
        taps = [(kz - (kz_n // 2), ky - 1, kx - 1) for kz in range(kz_n) for ky in range(3) for kx in range(3)]
        return entry(w.reshape(Co, Ci, -1).permute(2, 1, 0).reshape(-1, Co), taps, Co)
    Co = w.shape[1]
    # the parity table of _kidx as (kernel index, input offset) -- with the odd class's offset-1 tap FIRST, the order this
    # kernel's tap lists have always had (which is why _parity_taps is not used here)
    dim_opts = {0: [(1, 0)], 1: [(0, 1), (2, 0)]}
    out = []
    for pz in ([0] if kz_n == 1 else [0, 1]):
        for py in (0, 1):
            for px in (0, 1):
                taps, cols = [], []
                for (kz, oz) in ([(0, 0)] if kz_n == 1 else dim_opts[pz]):
                    for (ky, oy) in dim_opts[py]:
                        for (kx, ox) in dim_opts[px]:
                            taps.append((oz, oy, ox))
                            cols.append(w[:, :, kz, ky, kx])  # [Ci, Co]
                out.append(((pz, py, px),) + entry(torch.stack(cols, 0).reshape(-1, Co), taps, Co))   # [T*Ci, Co]
    return out


# ----------------------------------------------------------------------------------------
# z-streaming folded implicit GEMM (d3d_conv_fold_f32): tap lists / packed weights per layer
# ----------------------------------------------------------------------------------------
def _dim_conv(K, stride, fold):
    """One dimension of an ordinary convolution (odd kernel size K, padding K // 2) folded over `fold`
    neighbouring outputs: (tap offsets, fold positions, k(tap, fold) -> kernel index or -1, input step, output
    step, base).  K = 0 marks the degenerate row dimension of an image (a single tap, a single position)."""
    if K == 0:
        return [0], [0], (lambda t, f: 0), 1, 1, 0
    pad = K // 2
    taps = list(range(-pad, (fold - 1) * stride + pad + 1))
    k = lambda t, f: (t - f * stride + pad) if 0 <= t - f * stride + pad < K else -1
    return taps, list(range(fold)), k, fold * stride, fold, 0


def _dim_convT(K, parities):
    """One dimension of a k=3 stride-2 pad-1 output_pad-1 transposed convolution: output 2g+p reads input
    g+o with kernel index k(o,p): p even -> (o=0: 1); p odd -> (o=0: 2, o=1: 0) -- _kidx, or -1."""
    if K == 0:
        return [0], [0], (lambda t, f: 0), 1, 1, 0
    k = lambda o, f: -1 if _kidx(3, parities[f], o) is None else _kidx(3, parities[f], o)
    return [0, 1], list(range(len(parities))), k, 1, 2, (parities[0] if len(parities) == 1 else 0)


def _fold_pack(wk, dims, Co, ksizes):
    """wk [Co,Ci,K0*K1*K2] (kernel sizes ksizes, in the streaming/row/column order of `dims`) ->
    (wpack [T,Ci,mpad], taps bytes (sorted by the first dimension), T, M, mpad, [c,s,b,f per dim])."""
    (t0, f0, k0, c0, s0, b0), (t1, f1, k1, c1, s1, b1), (t2, f2, k2, c2, s2, b2) = dims
    K1, K2 = ksizes[1], ksizes[2]
    F = len(f0) * len(f1) * len(f2)
    M = Co * F
    if M > 64:
        raise ValueError("fold %dx%dx%d of %d channels exceeds 64 GEMM rows" % (len(f0), len(f1), len(f2), Co))
    mpad = 16 if M <= 16 else (32 if M <= 32 else 64)
    nk = wk.shape[2]
    taps, kidx = [], []
    for o0 in t0:
        for o1 in t1:
            for o2 in t2:
                row = []
                for a in f0:
                    for b in f1:
                        for c in f2:
                            i, jj, l = k0(o0, a), k1(o1, b), k2(o2, c)
                            row.append(nk if min(i, jj, l) < 0 else (i * K1 + jj) * K2 + l)
                if any(r != nk for r in row):
                    taps.append((o0, o1, o2))
                    kidx.append(row)
    T = len(taps)
    Ci = wk.shape[1]
    wz = torch.cat([wk, torch.zeros((Co, Ci, 1), dtype=wk.dtype, device=wk.device)], 2)
    idx = torch.tensor(kidx, dtype=torch.long, device=wk.device)        # [T, F]
    a = wz[:, :, idx]                                                    # [Co, Ci, T, F]
    a = a.permute(2, 1, 3, 0).reshape(T, Ci, M)                          # row m = fold*Co + co
    wpack = torch.zeros((T, Ci, mpad), dtype=torch.float32, device=wk.device)
    wpack[:, :, :M] = a
    tail = [c0, c1, c2, s0, s1, s2, b0, b1, b2, len(f0), len(f1), len(f2)]
    return wpack.contiguous(), _np.array(taps, _np.int8).tobytes(), T, M, mpad, tail


def _conv_fold_choice(Co, Ci, three_d, stride, K=3):
    """Fold (f_y, f_x) that fills the 16 GEMM rows of a narrow layer.  Limits: the kernel's 128 taps, and resident
    weights (ntaps * Ci * 16 floats) small enough that two workgroups still share a CU's LDS -- a wide-C_in layer
    is faster unfolded at twice the occupancy (stage-1 conv0 32->8: 9.4 ms folded, 5.3 ms unfolded)."""
    budget = 48 * 1024
    ntaps = lambda f: (K if three_d else 1) * ((f[0] - 1) * stride + K) * ((f[1] - 1) * stride + K)
    for f in [(4, 4), (2, 4), (2, 2), (1, 2)]:
        # (the kernel's column step f_x * stride must be 1, 2 or 4)
        if Co * f[0] * f[1] <= 16 and f[1] * stride <= 4 and ntaps(f) <= 128 and ntaps(f) * Ci * 64 <= budget:
            return f
    return (1, 1)


def _pack_fold(weight, transposed, stride):
    """List of launches [(wpack, taps, T, M, mpad, geom tail)] for one layer (_runtime._packed_fold caches them).

    Dimension order of the kernel is (streamed, row, column).  A volume [C,D,H,W] maps (z, y, x) onto it; an
    image [C,H,W] is handed over as [C, H, 1, W] -- its rows are the streamed planes, so every input row is
    staged once and the kernel's z machinery (open accumulator sets, z fold) serves the image's y axis."""
    w = weight.float()
    three_d = w.dim() == 5
    if transposed:
        w = w.transpose(0, 1)
    Co, Ci = w.shape[0], w.shape[1]
    wk = w.reshape(Co, Ci, -1).contiguous()
    K = w.shape[-1]  # cubic / square kernels, odd size, padding K // 2 (1, 3 and 5 occur in the reference)
    if K % 2 == 0 or any(d != K for d in w.shape[2:]) or (transposed and K != 3):
        raise ValueError("unsupported kernel shape %s" % (tuple(w.shape[2:]),))
    ks = (K, K, K) if three_d else (K, 1, K)
    if not transposed:
        fy, fx = _conv_fold_choice(Co, Ci, three_d, stride, K)
        if three_d:
            dims = (_dim_conv(K, stride, 1), _dim_conv(K, stride, fy), _dim_conv(K, stride, fx))
        else:
            dims = (_dim_conv(K, stride, fy), _dim_conv(0, 1, 1), _dim_conv(K, stride, fx))
        return [_fold_pack(wk, dims, Co, ks)]
    # all output parities as GEMM rows while they fit 64 rows; otherwise one launch per parity of the
    # leading dimensions
    ks0 = [k if k == 3 else 0 for k in ks]
    sets = [[[0, 1]] if k == 3 else [None] for k in ks]
    rows = lambda: Co * int(_np.prod([len(ss[0]) if ss[0] else 1 for ss in sets]))
    for d in range(3):
        if rows() > 64 and ks[d] == 3:
            sets[d] = [[0], [1]]
    return [_fold_pack(wk, tuple(_dim_convT(ks0[d], pp) for d, pp in enumerate((p0, p1, p2))), Co, ks)
            for p0 in sets[0] for p1 in sets[1] for p2 in sets[2]]
