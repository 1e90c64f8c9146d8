// Rigid registration of a point cloud to a reference cloud (iterative closest point): the two kernels around the capped search of
// cloud_compare.hip (deep3d_aerial_amd/cloud_register.py states the rule, include/deep3d_planesweep.h too,
// tests/cloud_register_scene.py restates it in numpy).  The rule is this project's own; it does not claim to match any tool.
//
// Transform.  T is 3 x 4 fp64, row-major, in DEVICE memory.  Per point (x, y, z) fp32 and output row r:
//   p'_r = (float)(((T[r][0] (double)x + T[r][1] (double)y) + T[r][2] (double)z) + T[r][3])
// every operation fp64 and rounded once (-ffp-contract=off), the result rounded once to fp32.  A non-finite input gives whatever
// that arithmetic gives; the keys drop such a point later.  The caller transforms the ORIGINAL cloud by the accumulated T every
// iteration, so fp32 roundings never pile up.
//
// Sums.  Of the moved cloud P' [n,3], its e [n] and idx [n] from d3d_cloud_compare_nearest against the reference Q [m,3] on the
// grid of cap h with origin o = (xmin, ymin, zmin).  Pair i counts when 0 <= idx_i < m and e_i <= e_max.  Per counted pair
//   a_c = llrint(((double)p'_c - o_c) / h * 1024.0),   b_c likewise from Q[idx_i]        (1024ths of a cap from the origin)
// A keyed point lies inside a grid of at most 2^21 - 1 cells per axis, so 0 <= a_c, b_c < 2^31 and a_r b_c < 2^62.
// sums int64 [27], zeroed by the call:
//   [0] N = the counted pairs   [1..3] sum a   [4..6] sum b   [7..15] sum (a_r b_c) & 0xFFFFFFFF, row-major
//   [16..24] sum (a_r b_c) >> 32   [25] sum e   [26] sum e^2
// With at most 2^31 - 1 points no slot overflows (a plain 64-bit sum of the products would wrap at four points in the far corner
// of a large grid: the split is the point of the layout); the host recombines M_rc = hi 2^32 + lo in unbounded integers.
//
// transform: one lane per four points: three 16-byte loads and three 16-byte stores where both arrays are 16-byte aligned, twelve
//            4-byte ones otherwise (a view that starts at a row other than the first); 24 bytes a point, bandwidth-bound.
// sums:      a grid-stride loop over the pairs by as many workgroups as are resident at once (at most CR_GRID_CAP; the lesson of
//            §4.29).  Every lane keeps its 27 partial sums in registers (54 VGPRs; a lane sees at most 2^31 / lanes pairs, so the
//            split limbs cannot overflow in a lane either).  At its end a workgroup reduces once: shuffles within a wave, LDS
//            across its four waves, then one set of 27 global integer atomicAdd.
// Atomics: that one integer atomicAdd, result unused: the same bits for any order of the pairs.
//
// Plane sums.  The same pairs with the reference's normals N [m,3] fp32, for the point-to-plane metric.
// c_c = 512 n_c is the grid's centre in bins; m_c = llrint((double)N[idx_i]_c * 1024.0).  Pair i counts when it counts above and its
// normal is finite with every |component| <= 1 and m != (0, 0, 0).  Per counted pair
//   u = a - c,   r = (a - b) . m,   w = u x m,   g = (w_x, w_y, w_z, m_x, m_y, m_z)
// and the residual linearised under a rotation omega about c and a translation tau (in bins) is r + g . (omega, tau).
// sums int64 [87], zeroed by the call: [0] N, [1] sum e, [2] sum e^2, then 28 products P_k -- the 21 g_i g_j, i <= j, row-major; the
// 6 g_i r; r r --, each a 128-bit two's-complement value summed in three slots 3 + 3k .. 5 + 3k: the low 32 bits of its low word, the
// high 32 bits of its low word (both unsigned), its signed high word: the split above with one more limb, for the same reason.
// |w| < 2^42, |r| < 2^43, |P| < 2^87; 2^31 - 1 pairs overflow no slot; the host recombines in unbounded integers.
// plane sums: the loop of the sums with 87 partial sums a lane (256 VGPRs and 108 AGPRs, no scratch, one wave per SIMD) and the
//            same reduction (cr_reduce).
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CR_BLOCK = 256;
constexpr int CR_WAVES = CR_BLOCK / 64;
constexpr int CR_POINTS = 4;         // points per lane of the transform: 48 bytes, three 16-byte accesses
constexpr int CR_SUMS = 27;
constexpr int CR_GRID_CAP = 2048;    // workgroups of the sums launched at most (fewer where fewer are resident)
constexpr int CR_PLANE_SUMS = 87;    // N, sum e, sum e^2 and 28 products of three limbs each

// Row r of the transform: ((t0 x + t1 y) + t2 z) + t3 in fp64, each operation rounded once, then rounded to fp32.
__device__ __forceinline__ float cr_row(const double* t, double x, double y, double z) { return (float)(((t[0] * x + t[1] * y) + t[2] * z) + t[3]); }

__device__ __forceinline__ void cr_point(const double* t, const float* v, float* w) {
    const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
    w[0] = cr_row(t, x, y, z);
    w[1] = cr_row(t + 4, x, y, z);
    w[2] = cr_row(t + 8, x, y, z);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CR_BLOCK) void cloud_transform_kernel(const float* __restrict__ xyz, long n, const double* __restrict__ rt,
                                                                   float* __restrict__ out) {
    const long g = (long)blockIdx.x * CR_BLOCK + threadIdx.x;   // this lane's group of CR_POINTS points
    const long first = g * CR_POINTS;
    if (first >= n) return;
    double t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = rt[k];
    if (first + CR_POINTS <= n) {
        float v[3 * CR_POINTS], w[3 * CR_POINTS];
        if (ALIGNED) {
            const float4* src = (const float4*)(xyz + 3 * first);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 a = src[k];
                v[4 * k] = a.x, v[4 * k + 1] = a.y, v[4 * k + 2] = a.z, v[4 * k + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * CR_POINTS; ++k) v[k] = xyz[3 * first + k];
        }
#pragma unroll
        for (int p = 0; p < CR_POINTS; ++p) cr_point(t, v + 3 * p, w + 3 * p);
        if (ALIGNED) {
            float4* dst = (float4*)(out + 3 * first);
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 3 * CR_POINTS; ++k) out[3 * first + k] = w[k];
        }
    } else {   // the last group of a cloud whose size is no multiple of CR_POINTS
        for (long p = first; p < n; ++p) {
            const float v[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
            float w[3];
            cr_point(t, v, w);
            out[3 * p] = w[0], out[3 * p + 1] = w[1], out[3 * p + 2] = w[2];
        }
    }
}

// A coordinate in 1024ths of a cap from the grid's origin.
__device__ __forceinline__ long long cr_bin(float v, double o, double h) { return llrint(((double)v - o) / h * 1024.0); }

// The N partial sums of every lane of the workgroup into sums[0 .. N - 1]: shuffles within a wave, LDS across the waves, then one
// integer atomicAdd per sum, its result unused.  Every lane of the workgroup calls it, once.
template <int N>
__device__ __forceinline__ void cr_reduce(const long long (&s)[N], unsigned long long* __restrict__ sums) {
    __shared__ long long part[CR_WAVES][N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long v = wave_sum(s[k]);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (tid < N) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < CR_WAVES; ++w) v += part[w][tid];
        atomicAdd(sums + tid, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(CR_BLOCK) void cloud_register_sums_kernel(const float* __restrict__ q_xyz, const int* __restrict__ e,
                                                                       const int* __restrict__ idx, long nq, const float* __restrict__ t_xyz,
                                                                       long nt, double ox, double oy, double oz, double h, int e_max,
                                                                       unsigned long long* __restrict__ sums) {
    long long s[CR_SUMS];
#pragma unroll
    for (int k = 0; k < CR_SUMS; ++k) s[k] = 0;
    const long stride = (long)gridDim.x * CR_BLOCK;
    for (long i = (long)blockIdx.x * CR_BLOCK + threadIdx.x; i < nq; i += stride) {
        const int ei = e[i];
        const long j = idx[i];
        if (j < 0 || j >= nt || ei > e_max) continue;   // not a counted pair; an idx outside the reference is never dereferenced
        const long long a[3] = {cr_bin(q_xyz[3 * i], ox, h), cr_bin(q_xyz[3 * i + 1], oy, h), cr_bin(q_xyz[3 * i + 2], oz, h)};
        const long long b[3] = {cr_bin(t_xyz[3 * j], ox, h), cr_bin(t_xyz[3 * j + 1], oy, h), cr_bin(t_xyz[3 * j + 2], oz, h)};
        s[0] += 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[1 + c] += a[c];
            s[4 + c] += b[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long m = a[r] * b[c];
                s[7 + 3 * r + c] += m & 0xFFFFFFFFll;
                s[16 + 3 * r + c] += m >> 32;
            }
        s[25] += ei;
        s[26] += (long long)ei * ei;
    }
    cr_reduce<CR_SUMS>(s, sums);
}

// One 128-bit product x y into its three slots: the low and the high 32 bits of the low word (unsigned) and the signed high word.
// wide = false (a constant at every call once the loops are unrolled): the caller knows |x y| < 2^63 (a factor is a normal's component, |m| <= 1024, the other below 2^43), so the high
// word is the sign of the 64-bit product -- the same bits without the multiply for it.
__device__ __forceinline__ void cr_product(long long* s, long long x, long long y, bool wide) {
    const unsigned long long lo = (unsigned long long)x * (unsigned long long)y;
    s[0] += (long long)(lo & 0xFFFFFFFFull);
    s[1] += (long long)(lo >> 32);
    s[2] += wide ? __mul64hi(x, y) : ((long long)lo >> 63);
}

__global__ __launch_bounds__(CR_BLOCK) void cloud_register_plane_sums_kernel(const float* __restrict__ q_xyz, const int* __restrict__ e,
                                                                             const int* __restrict__ idx, long nq,
                                                                             const float* __restrict__ t_xyz,
                                                                             const float* __restrict__ t_normals, long nt, long long cx,
                                                                             long long cy, long long cz, double ox, double oy, double oz,
                                                                             double h, int e_max, unsigned long long* __restrict__ sums) {
    long long s[CR_PLANE_SUMS];
#pragma unroll
    for (int k = 0; k < CR_PLANE_SUMS; ++k) s[k] = 0;
    const long stride = (long)gridDim.x * CR_BLOCK;
    for (long i = (long)blockIdx.x * CR_BLOCK + threadIdx.x; i < nq; i += stride) {
        const int ei = e[i];
        const long j = idx[i];
        if (j < 0 || j >= nt || ei > e_max) continue;   // not a counted pair; an idx outside the reference is never dereferenced
        const double nd[3] = {(double)t_normals[3 * j] * 1024.0, (double)t_normals[3 * j + 1] * 1024.0, (double)t_normals[3 * j + 2] * 1024.0};
        if (!(fabs(nd[0]) <= 1024.0 && fabs(nd[1]) <= 1024.0 && fabs(nd[2]) <= 1024.0)) continue;   // not finite, or longer than a unit normal
        const long long m[3] = {llrint(nd[0]), llrint(nd[1]), llrint(nd[2])};
        if ((m[0] | m[1] | m[2]) == 0) continue;
        const long long a[3] = {cr_bin(q_xyz[3 * i], ox, h), cr_bin(q_xyz[3 * i + 1], oy, h), cr_bin(q_xyz[3 * i + 2], oz, h)};
        const long long b[3] = {cr_bin(t_xyz[3 * j], ox, h), cr_bin(t_xyz[3 * j + 1], oy, h), cr_bin(t_xyz[3 * j + 2], oz, h)};
        const long long u[3] = {a[0] - cx, a[1] - cy, a[2] - cz};
        const long long r = ((a[0] - b[0]) * m[0] + (a[1] - b[1]) * m[1]) + (a[2] - b[2]) * m[2];
        const long long g[7] = {u[1] * m[2] - u[2] * m[1], u[2] * m[0] - u[0] * m[2], u[0] * m[1] - u[1] * m[0], m[0], m[1], m[2], r};
        s[0] += 1;
        s[1] += ei;
        s[2] += (long long)ei * ei;
        int k = 3;   // (a compile-time constant at every use once the loops are unrolled)
#pragma unroll
        for (int r0 = 0; r0 < 6; ++r0)
#pragma unroll
            for (int c0 = r0; c0 < 6; ++c0, k += 3) cr_product(s + k, g[r0], g[c0], r0 < 3 && c0 < 3);   // w w alone is wide
#pragma unroll
        for (int r0 = 0; r0 < 7; ++r0, k += 3) cr_product(s + k, g[r0], g[6], r0 < 3 || r0 == 6);   // w r and r r
    }
    cr_reduce<CR_PLANE_SUMS>(s, sums);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------

static int reg_resident(int* out) {
    static int known[SEARCH_MAX_DEVICES] = {};
    return search_resident((const void*)cloud_register_sums_kernel, CR_BLOCK, CR_GRID_CAP, known, "cloud register: resident workgroups", out);
}

static int reg_plane_resident(int* out) {
    static int known[SEARCH_MAX_DEVICES] = {};
    return search_resident((const void*)cloud_register_plane_sums_kernel, CR_BLOCK, CR_GRID_CAP, known,
                           "cloud register: resident workgroups of the plane sums", out);
}

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_cloud_transform(const float* xyz, long long n, const double* rt, float* out, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n), "n=%lld (0 .. 2^31 - 1)", n);
    D3D_REQUIRE((xyz && rt && out) || n == 0, "null pointer (xyz, rt, out) with %lld points", n);
    const SearchRange R[3] = {{xyz, (size_t)n * 12}, {rt, n ? (size_t)96 : 0}, {out, (size_t)n * 12}};
    D3D_REQUIRE(search_apart(R, 3), "xyz, rt and out must not alias");
    if (n == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(ceil_div(n, CR_POINTS), CR_BLOCK));
    if ((((uintptr_t)xyz | (uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL(cloud_transform_kernel<true>, grid, dim3(CR_BLOCK), 0, st, xyz, (long)n, rt, out);
    else
        hipLaunchKernelGGL(cloud_transform_kernel<false>, grid, dim3(CR_BLOCK), 0, st, xyz, (long)n, rt, out);
    D3D_LAUNCH_CHECK("cloud_transform_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_cloud_register_sums(const float* q_xyz, const int* e, const int* idx, long long n_query, const float* t_xyz,
                                       long long n_target, double xmin, double ymin, double zmin, double cap, int e_max, long long* sums,
                                       d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_query), "n_query=%lld (0 .. 2^31 - 1)", n_query);
    D3D_REQUIRE(count_ok(n_target), "n_target=%lld (0 .. 2^31 - 1)", n_target);
    D3D_REQUIRE(sums, "null pointer (sums)");
    D3D_REQUIRE((q_xyz && e && idx) || n_query == 0, "null pointer (q_xyz, e, idx) with %lld queries", n_query);
    D3D_REQUIRE(t_xyz || n_target == 0, "null pointer (t_xyz) with %lld targets", n_target);
    D3D_REQUIRE(std::isfinite(xmin) && std::isfinite(ymin) && std::isfinite(zmin), "origin (%g, %g, %g) must be finite", xmin, ymin, zmin);
    if (search_cap_ok(cap) != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(e_max >= 0 && e_max <= CLOUD_E_CAP, "e_max=%d (0 .. 1024)", e_max);
    const size_t nq = (size_t)n_query, nt = (size_t)n_target;
    const SearchRange R[5] = {{q_xyz, nq * 12}, {e, nq * 4}, {idx, nq * 4}, {t_xyz, nt * 12}, {sums, (size_t)CR_SUMS * 8}};
    D3D_REQUIRE(search_apart(R, 5), "q_xyz, e, idx, t_xyz and sums must not alias");
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(sums, 0, (size_t)CR_SUMS * 8, st), "cloud register: clear sums");
    if (rc != D3D_OK) return rc;
    if (n_query == 0 || n_target == 0) return D3D_OK;   // no pair can count
    int resident = 0;
    const int rc2 = reg_resident(&resident);
    if (rc2 != D3D_OK) return rc2;
    const long n_blocks = (long)((n_query + CR_BLOCK - 1) / CR_BLOCK);
    const dim3 grid((unsigned)(n_blocks < resident ? n_blocks : resident));
    hipLaunchKernelGGL(cloud_register_sums_kernel, grid, dim3(CR_BLOCK), 0, st, q_xyz, e, idx, (long)n_query, t_xyz, (long)n_target, xmin, ymin,
                       zmin, cap, e_max, (unsigned long long*)sums);
    D3D_LAUNCH_CHECK("cloud_register_sums_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_cloud_register_plane_sums(const float* q_xyz, const int* e, const int* idx, long long n_query, const float* t_xyz,
                                             const float* t_normals, long long n_target, int nx, int ny, int nz, double xmin, double ymin,
                                             double zmin, double cap, int e_max, long long* sums, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_query), "n_query=%lld (0 .. 2^31 - 1)", n_query);
    D3D_REQUIRE(count_ok(n_target), "n_target=%lld (0 .. 2^31 - 1)", n_target);
    D3D_REQUIRE(sums, "null pointer (sums)");
    D3D_REQUIRE((q_xyz && e && idx) || n_query == 0, "null pointer (q_xyz, e, idx) with %lld queries", n_query);
    D3D_REQUIRE((t_xyz && t_normals) || n_target == 0, "null pointer (t_xyz, t_normals) with %lld targets", n_target);
    if (search_grid_ok(nx, ny, nz, "cells") != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(std::isfinite(xmin) && std::isfinite(ymin) && std::isfinite(zmin), "origin (%g, %g, %g) must be finite", xmin, ymin, zmin);
    if (search_cap_ok(cap) != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(e_max >= 0 && e_max <= CLOUD_E_CAP, "e_max=%d (0 .. 1024)", e_max);
    const size_t nq = (size_t)n_query, nt = (size_t)n_target;
    const SearchRange R[6] = {{q_xyz, nq * 12}, {e, nq * 4}, {idx, nq * 4}, {t_xyz, nt * 12}, {t_normals, nt * 12}, {sums, (size_t)CR_PLANE_SUMS * 8}};
    D3D_REQUIRE(search_apart(R, 6), "q_xyz, e, idx, t_xyz, t_normals and sums must not alias");
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(sums, 0, (size_t)CR_PLANE_SUMS * 8, st), "cloud register: clear plane sums");
    if (rc != D3D_OK) return rc;
    if (n_query == 0 || n_target == 0) return D3D_OK;   // no pair can count
    int resident = 0;
    const int rc2 = reg_plane_resident(&resident);
    if (rc2 != D3D_OK) return rc2;
    const long n_blocks = (long)((n_query + CR_BLOCK - 1) / CR_BLOCK);
    const dim3 grid((unsigned)(n_blocks < resident ? n_blocks : resident));
    hipLaunchKernelGGL(cloud_register_plane_sums_kernel, grid, dim3(CR_BLOCK), 0, st, q_xyz, e, idx, (long)n_query, t_xyz, t_normals,
                       (long)n_target, 512ll * nx, 512ll * ny, 512ll * nz, xmin, ymin, zmin, cap, e_max, (unsigned long long*)sums);
    D3D_LAUNCH_CHECK("cloud_register_plane_sums_kernel launch");
    return D3D_OK;
}
