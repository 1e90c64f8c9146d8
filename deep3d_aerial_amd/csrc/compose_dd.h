// module.py:528-530 for one source view: src_proj @ inverse(ref_proj), fp32 in and out, the arithmetic between in double-double.
// Host and device: compose_kernel (planesweep.hip) calls it per source view; nothing else here touches the GPU.
//
// Why not plain fp64.  The inputs are fp32 values, so the composition has one exact rational value per entry, and a world-frame
// camera (K [R|t] with every entry of R in play, |t| of 1e5 .. 1e8) makes some of those entries the remainder of a cancellation:
// a rotation entry that is zero for the ideal cameras comes out as the 1e-13 the rounding of the inputs left of terms of 1e-3.
// fp64 gets such an entry to 1e-16 of the TERMS, which is more than an fp32 ulp of the ENTRY (1.7 ulp on a 688 x 464 frame at
// f = 1750 px: tests/test_camera_ref.py restates it), though far below anything the image sees.  A double-double carries ~106 bits,
// so every entry is the fp32 rounding of the exact value unless the cancellation is deeper than 1e-22 of its terms
// (tests/test_world_cameras_gpu.py holds the kernel to one ulp of exact rational arithmetic).  One lane per view, once per stage.
//
// A double-double is an unevaluated sum hi + lo with |lo| <= ulp(hi) / 2.  two_sum (Knuth) and two_prod (one fma) are error-free;
// the file is built with -ffp-contract=off -fno-fast-math (csrc/Makefile), which they rely on.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define D3D_DD_FN __host__ __device__ inline
#else
#define D3D_DD_FN inline
#endif

namespace d3d {

struct dd {
    double hi, lo;
};

D3D_DD_FN dd dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

D3D_DD_FN dd dd_fast_two_sum(double a, double b) {   // |a| >= |b|, or a == 0
    const double s = a + b;
    return {s, b - (s - a)};
}

D3D_DD_FN dd operator+(dd a, dd b) {
    dd s = dd_two_sum(a.hi, b.hi);
    const dd t = dd_two_sum(a.lo, b.lo);
    s = dd_fast_two_sum(s.hi, s.lo + t.hi);
    return dd_fast_two_sum(s.hi, s.lo + t.lo);
}

D3D_DD_FN dd operator-(dd a) { return {-a.hi, -a.lo}; }
D3D_DD_FN dd operator-(dd a, dd b) { return a + (-b); }

D3D_DD_FN dd operator*(dd a, dd b) {
    const double p = a.hi * b.hi;
    const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return dd_fast_two_sum(p, e);
}

D3D_DD_FN dd operator/(dd a, dd b) {   // three quotient digits: long division on the leading parts
    const double q1 = a.hi / b.hi;
    dd r = a - b * dd{q1, 0.0};
    const double q2 = r.hi / b.hi;
    r = r - b * dd{q2, 0.0};
    const double q3 = r.hi / b.hi;
    return dd_fast_two_sum(q1, q2) + dd{q3, 0.0};
}

// ref44, src44: row-major fp32 [4,4]; out12: row-major [3,4] = [rot | trans].  Cofactor inverse of ref44, the product with src44,
// one rounding to fp32.  A singular ref_proj gives inf / nan, as torch.inverse would raise.
D3D_DD_FN void compose_proj_dd(const float* ref44, const float* src44, float* out12) {
    dd m[16], inv[16];
    for (int k = 0; k < 16; ++k) m[k] = dd{(double)ref44[k], 0.0};
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] +
             m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] -
             m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] +
             m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] -
              m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] -
             m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] +
             m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] -
             m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] +
              m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] +
             m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] -
             m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] +
              m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] -
              m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] -
             m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] +
             m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] -
              m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] +
              m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const dd det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            dd acc = {0.0, 0.0};
            for (int k = 0; k < 4; ++k) acc = acc + dd{(double)src44[r * 4 + k], 0.0} * inv[k * 4 + c];
            acc = acc / det;
            out12[r * 4 + c] = (float)(acc.hi + acc.lo);
        }
}

}  // namespace d3d
