// Surface normals from a depth map: ComputeNormals.compute_normal_by_depth of the reference
// (mvs/mvs_cas/models/compute_normals.py:32-82), whose product the fusion step reads as {view}_normal.pfm
// (fuse/fusion_3d_normal.py:437-443, 491-498) and which nothing in the reference produces.
//
// Per pixel (x, y) at distance >= nei from every border, with P(x, y) = inv(K) (x d, y d, d):
//   the eight differences of the 3x3 stencil of step nei against the centre, with the reference's signs (:51-58),
//   four cross products (x1, y1), (x0, y0), (x0y1, x0y0), (x1y0, x1y1), each normalised, summed, normalised again;
//   the border band of width nei is 0 (F.pad, :80).  F.normalize is v / max(|v|, 1e-12): the four cross products are
//   normalised as v * rsq(max(v.v, 1e-24)), the same vector to an ulp, the sum with IEEE sqrt and division; v = 0 stays 0,
//   so an all-zero neighbourhood gives (0, 0, 0) as in the reference.
//
// Numerics.  The reference forms each point in fp32 (|P| ~ the depth) and subtracts neighbours whose footprint is a few
// thousandths of that, so its differences carry the rounding of the points.  Here a difference is formed without the
// points: with r = inv(K) (x, y, 1) the centre's ray and e = inv(K) (dx, dy, 0) the (constant) step of the ray to the
// neighbour,   P_a - P_c = d_a e + (d_a - d_c) r   -- the same quantity, where d_a - d_c is exact for neighbouring
// depths (Sterbenz) and no term is as large as a point.  Against a float64 evaluation of the reference's formula this
// is far more accurate than the reference itself (tests/test_normals*.py read the bound from the golden data).
//
// Bytes: 4 in, 12 out per pixel (+12 with the encoded map); the ≈190 VALU operations per pixel, not the bytes, set the measured
// rate (profiles/normals_bench.json).  A lane makes 4 consecutive pixels of one row: its three 12-byte pixels x 4 are three 16-byte stores, and the
// depth rows arrive as one 16-byte load plus the 2*nei neighbours per row (the stencil's re-reads hit the caches).
// Rows whose width is not a multiple of 4, or unaligned tensors, take the scalar form of the same kernel; both evaluate
// every pixel with the same function, so the results do not depend on the path, on B or on the launch shape.
// No atomics, no reduction: bit-reproducible.
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int NRM_MAX_B = 64;   // items per launch (inv(K) travels in the kernel arguments)

struct NormalsKinv {
    float k[NRM_MAX_B][9];
};

struct NrmVec {
    float x, y, z;
};

// Two rounded products, then the difference (no fma): a x (-a) -- the two differences towards zero-depth holes on opposite sides
// of the centre, both -P_c -- is exactly 0 as in the float64 formula, where an fma leaves one product's rounding error and
// normalises that into a spurious unit vector.
__device__ __forceinline__ NrmVec nrm_cross(NrmVec a, NrmVec b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

__device__ __forceinline__ NrmVec nrm_normalize(NrmVec v) {
    // F.normalize(v) = v / max(|v|, 1e-12); 1e-24 is a normal fp32 number, so v_rsq never sees a denormal
    const float s = fmaf(v.x, v.x, fmaf(v.y, v.y, v.z * v.z));
    const float r = __builtin_amdgcn_rsqf(fmaxf(s, 1e-24f));
    return {v.x * r, v.y * r, v.z * r};
}

// The last normalisation exactly as F.normalize states it (IEEE sqrt and division): the result is a unit vector to half an
// ulp per component, where v_rsq's ulp would be the whole error budget on maps whose reference error is itself a few ulp.
__device__ __forceinline__ NrmVec nrm_normalize_ieee(NrmVec v) {
    const float n = fmaxf(sqrtf(fmaf(v.x, v.x, fmaf(v.y, v.y, v.z * v.z))), 1e-12f);
    return {v.x / n, v.y / n, v.z / n};
}

// P_a - P_c = d_a e + (d_a - d_c) r
__device__ __forceinline__ NrmVec nrm_diff(float da, float dc, NrmVec e, NrmVec r) {
    const float dd = da - dc;
    return {fmaf(dd, r.x, da * e.x), fmaf(dd, r.y, da * e.y), fmaf(dd, r.z, da * e.z)};
}

struct NrmSteps {
    NrmVec ex, ey, epp, epm;   // inv(K) (nei, 0, 0), (0, nei, 0), (nei, nei, 0), (nei, -nei, 0)
};

__device__ __forceinline__ NrmSteps nrm_steps(const float* k, int nei) {
    const float s = (float)nei;
    NrmSteps t;
    t.ex = {s * k[0], s * k[3], s * k[6]};
    t.ey = {s * k[1], s * k[4], s * k[7]};
    t.epp = {t.ex.x + t.ey.x, t.ex.y + t.ey.y, t.ex.z + t.ey.z};
    t.epm = {t.ex.x - t.ey.x, t.ex.y - t.ey.y, t.ex.z - t.ey.z};
    return t;
}

__device__ __forceinline__ NrmVec neg(NrmVec v) { return {-v.x, -v.y, -v.z}; }

// The normal of one interior pixel from its 3x3 stencil: t = row y - nei, m = row y, b = row y + nei; [0] = x - nei,
// [1] = x, [2] = x + nei.
__device__ __forceinline__ NrmVec nrm_pixel(const float* k, const NrmSteps& st, float x, float y, float t0, float t1, float t2,
                                            float m0, float m1, float m2, float b0, float b1, float b2) {
    const NrmVec r = {fmaf(k[0], x, fmaf(k[1], y, k[2])), fmaf(k[3], x, fmaf(k[4], y, k[5])), fmaf(k[6], x, fmaf(k[7], y, k[8]))};
    const float c = m1;
    // compute_normals.py:51-58 (a "-" on D(a) = P_a - P_ctr where the reference subtracts the other way round)
    const NrmVec diff_x0 = neg(nrm_diff(m0, c, neg(st.ex), r));
    const NrmVec diff_x1 = neg(nrm_diff(m2, c, st.ex, r));
    const NrmVec diff_y0 = nrm_diff(t1, c, neg(st.ey), r);
    const NrmVec diff_y1 = nrm_diff(b1, c, st.ey, r);
    const NrmVec diff_x0y0 = nrm_diff(t0, c, neg(st.epp), r);
    const NrmVec diff_x0y1 = neg(nrm_diff(b0, c, neg(st.epm), r));
    const NrmVec diff_x1y0 = nrm_diff(t2, c, st.epm, r);
    const NrmVec diff_x1y1 = neg(nrm_diff(b2, c, st.epp, r));
    // :70-77
    const NrmVec n0 = nrm_normalize(nrm_cross(diff_x1, diff_y1));
    const NrmVec n1 = nrm_normalize(nrm_cross(diff_x0, diff_y0));
    const NrmVec n2 = nrm_normalize(nrm_cross(diff_x0y1, diff_x0y0));
    const NrmVec n3 = nrm_normalize(nrm_cross(diff_x1y0, diff_x1y1));
    const NrmVec s = {((n0.x + n1.x) + n2.x) + n3.x, ((n0.y + n1.y) + n2.y) + n3.y, ((n0.z + n1.z) + n2.z) + n3.z};
    return nrm_normalize_ieee(s);
}

// NEI > 0 && VEC: W % 4 == 0 and 16-byte aligned tensors, nei == NEI.  Otherwise (NEI = 0) scalar loads and stores, any nei.
template <int NEI, bool VEC>
__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ depth, NormalsKinv kinv, int b0, int H, int W,
                                                      int nei_rt, float* __restrict__ normal, float* __restrict__ encoded) {
    const int nei = NEI > 0 ? NEI : nei_rt;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y, b = b0 + blockIdx.z;
    if (x0 >= W || y >= H) return;
    const float* k = kinv.k[blockIdx.z];
    const long pix = ((long)b * H + y) * W + x0;
    float o[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = 0.0f;
    if (y >= nei && y < H - nei) {
        const NrmSteps st = nrm_steps(k, nei);
        const float* rt = depth + ((long)b * H + y - nei) * W;
        const float* rm = rt + (long)nei * W;
        const float* rb = rm + (long)nei * W;
        if constexpr (VEC) {
            // row values at x0 - NEI .. x0 + 3 + NEI
            float t[4 + 2 * NEI], m[4 + 2 * NEI], bb[4 + 2 * NEI];
            const float4 tv = *reinterpret_cast<const float4*>(rt + x0), mv = *reinterpret_cast<const float4*>(rm + x0),
                         bv = *reinterpret_cast<const float4*>(rb + x0);
            t[NEI] = tv.x; t[NEI + 1] = tv.y; t[NEI + 2] = tv.z; t[NEI + 3] = tv.w;
            m[NEI] = mv.x; m[NEI + 1] = mv.y; m[NEI + 2] = mv.z; m[NEI + 3] = mv.w;
            bb[NEI] = bv.x; bb[NEI + 1] = bv.y; bb[NEI + 2] = bv.z; bb[NEI + 3] = bv.w;
#pragma unroll
            for (int j = 0; j < NEI; ++j) {
                const int xl = x0 - NEI + j, xr = x0 + 4 + j;
                t[j] = xl >= 0 ? rt[xl] : 0.0f;
                m[j] = xl >= 0 ? rm[xl] : 0.0f;
                bb[j] = xl >= 0 ? rb[xl] : 0.0f;
                t[NEI + 4 + j] = xr < W ? rt[xr] : 0.0f;
                m[NEI + 4 + j] = xr < W ? rm[xr] : 0.0f;
                bb[NEI + 4 + j] = xr < W ? rb[xr] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int x = x0 + i;
                if (x >= NEI && x < W - NEI) {
                    const NrmVec n = nrm_pixel(k, st, (float)x, (float)y, t[i], t[i + NEI], t[i + 2 * NEI], m[i], m[i + NEI],
                                               m[i + 2 * NEI], bb[i], bb[i + NEI], bb[i + 2 * NEI]);
                    o[3 * i] = n.x;
                    o[3 * i + 1] = n.y;
                    o[3 * i + 2] = n.z;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int x = x0 + i;
                if (x >= nei && x < W - nei) {
                    const int xl = x - nei, xr = x + nei;
                    const NrmVec n = nrm_pixel(k, st, (float)x, (float)y, rt[xl], rt[x], rt[xr], rm[xl], rm[x], rm[xr], rb[xl],
                                               rb[x], rb[xr]);
                    o[3 * i] = n.x;
                    o[3 * i + 1] = n.y;
                    o[3 * i + 2] = n.z;
                }
            }
        }
    }
    if constexpr (VEC) {
        if (normal) {
            float4* p = reinterpret_cast<float4*>(normal + 3 * pix);
            p[0] = make_float4(o[0], o[1], o[2], o[3]);
            p[1] = make_float4(o[4], o[5], o[6], o[7]);
            p[2] = make_float4(o[8], o[9], o[10], o[11]);
        }
        if (encoded) {   // (n + 1) / 2: the payload of {view}_normal.pfm (read_normal, fusion_3d_normal.py:191-195: x * 2 - 1)
            float4* p = reinterpret_cast<float4*>(encoded + 3 * pix);
            p[0] = make_float4((o[0] + 1.0f) * 0.5f, (o[1] + 1.0f) * 0.5f, (o[2] + 1.0f) * 0.5f, (o[3] + 1.0f) * 0.5f);
            p[1] = make_float4((o[4] + 1.0f) * 0.5f, (o[5] + 1.0f) * 0.5f, (o[6] + 1.0f) * 0.5f, (o[7] + 1.0f) * 0.5f);
            p[2] = make_float4((o[8] + 1.0f) * 0.5f, (o[9] + 1.0f) * 0.5f, (o[10] + 1.0f) * 0.5f, (o[11] + 1.0f) * 0.5f);
        }
    } else {
        const int n = W - x0 < 4 ? W - x0 : 4;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            if (i < 3 * n) {
                if (normal) normal[3 * pix + i] = o[i];
                if (encoded) encoded[3 * pix + i] = (o[i] + 1.0f) * 0.5f;
            }
        }
    }
}

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_normals_from_depth(const float* depth, const float* kinv, int B, int H, int W, int nei, float* normal,
                                      float* encoded, d3d_stream_t stream) {
    D3D_REQUIRE(depth && kinv, "null pointer (depth, kinv)");
    D3D_REQUIRE(normal || encoded, "null pointer: no output (normal and encoded both NULL)");
    D3D_REQUIRE(B >= 1 && H >= 1 && W >= 1, "bad dims B=%d %dx%d", B, H, W);
    D3D_REQUIRE(nei >= 1, "nei=%d (>= 1)", nei);
    D3D_REQUIRE(H >= 2 * nei && W >= 2 * nei, "map %dx%d smaller than the stencil (2*nei = %d)", H, W, 2 * nei);
    D3D_REQUIRE((long)ceil_div(H, 4) <= 65535, "H=%d too large", H);
    const size_t in_bytes = (size_t)B * H * W * sizeof(float), out_bytes = 3 * in_bytes;
    // (an output that is NULL is not written)
    D3D_REQUIRE((!normal || geom_apart(depth, in_bytes, normal, out_bytes)) && (!encoded || geom_apart(depth, in_bytes, encoded, out_bytes)) &&
                    (!normal || !encoded || geom_apart(normal, out_bytes, encoded, out_bytes)),
                "outputs must not alias the depth map or each other");
    for (int i = 0; i < 9 * B; ++i) D3D_REQUIRE(std::isfinite(kinv[i]), "inv(K) of item %d is not finite", i / 9);
    const bool vec = W % 4 == 0 && ((uintptr_t)depth & 15) == 0 && ((uintptr_t)normal & 15) == 0 && ((uintptr_t)encoded & 15) == 0;
    const dim3 block(64, 4);
    const int gx = ceil_div(ceil_div(W, 4), 64), gy = ceil_div(H, 4);
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += NRM_MAX_B) {
        const int nb = B - b0 < NRM_MAX_B ? B - b0 : NRM_MAX_B;
        NormalsKinv k = {};
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j < 9; ++j) k.k[i][j] = kinv[(size_t)(b0 + i) * 9 + j];
        const dim3 grid(gx, gy, nb);
        if (vec && nei == 1)
            hipLaunchKernelGGL((normals_kernel<1, true>), grid, block, 0, st, depth, k, b0, H, W, nei, normal, encoded);
        else if (vec && nei == 2)
            hipLaunchKernelGGL((normals_kernel<2, true>), grid, block, 0, st, depth, k, b0, H, W, nei, normal, encoded);
        else
            hipLaunchKernelGGL((normals_kernel<0, false>), grid, block, 0, st, depth, k, b0, H, W, nei, normal, encoded);
        D3D_LAUNCH_CHECK("normals_kernel launch");
    }
    return D3D_OK;
}
