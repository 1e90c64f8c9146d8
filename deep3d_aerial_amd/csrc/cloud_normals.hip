// Normals of a point cloud from its own neighbourhoods: a plane fitted to the points within a radius (DESIGN.md §4.34;
// deep3d_aerial_amd/cloud_normals.py states the rule, include/deep3d_planesweep.h too, tests/cloud_normals_scene.py restates it
// in numpy).  The rule is this project's own; it does not claim to match any tool.
//
// Grid: the cloud's (cloud.hip), one cell one radius h wide; a point is keyed by d3d_cloud_keys.  A point it drops is unkeyed:
// count 0, normal (0, 0, 0), flatness -1, nobody's neighbour.
// Per keyed point i the neighbours are the keyed points j, i itself included, of the 3 x 3 x 3 cells around i's cell with
//   d2 = cloud_d2(i, j) < h h                    (strict, fp64, each operation rounded once: -ffp-contract=off)
// Per neighbour and axis  delta_c = llrint(((double)x_jc - (double)x_ic) / h * 1024.0), so |delta_c| <= 1024.
// Ten integer sums, int64: k (the neighbours), S1[3] = sum delta, S2[6] = sum delta_r delta_c for rc = xx xy xz yy yz zz.
// k < 2^31 and |S2| < 2^51: nothing overflows, and integers sum to the same bits in any order.
// Covariance, fp64, each operation rounded once:  C_rc = (double)S2_rc - ((double)S1_r * (double)S1_c) / (double)k.
// Eigenvalues l0 <= l1 <= l2 of C and the unit eigenvector n of l0 by NORMALS_SWEEPS cyclic Jacobi sweeps (rotations (x, y),
// (x, z), (y, z) in that order; a zero off-diagonal entry is skipped), all in named fp64 registers: n is a function of the ten
// integers only.  n is flipped so that n . up >= 0, up = (0, 0, 1), or (0, 0, -1) with z_down; where n . up == 0 its first
// non-zero component is made positive.
// Outputs in input order: normal [n,3] fp32, count [n] int32 = k, flatness [n] int32 = llrint(1024 l0 / (l0 + l1 + l2)).
// Degenerate -- k < 3, or l2 <= 0, or l1 <= 1e-12 l2 (collinear) --: normal (0, 0, 0), flatness -1, count k.
//
// gather:  search_gather (cloud_search.h): the coordinates in key order as 16-byte records.
// normals: one lane per sorted point, one workgroup per SEARCH_BLOCK consecutive sorted points; search_tile parks the bounds of
//          the workgroup's cells in LDS and search_walk streams the candidates (the walk of cloud_outliers.hip).  The ten sums
//          stay in registers; the solve runs once per lane after the walk; the results go back through the order.
// Atomics: none.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int NORMALS_SWEEPS = 6;   // cyclic Jacobi converges quadratically: a 3 x 3 matrix is diagonal to fp64 after four
constexpr int NORMALS_SUMS = 10;

// One Jacobi rotation that zeroes the off-diagonal entry apq: app, aqq the two diagonal entries, arp and arq the entries that
// couple the third index to p and q, (v?p, v?q) the two columns of the eigenvector matrix.
__device__ __forceinline__ void normals_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                               double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // 0 for a theta past the range
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp, arq = rq;
    const double x0 = c * v0p - s * v0q, y0 = s * v0p + c * v0q;
    v0p = x0, v0q = y0;
    const double x1 = c * v1p - s * v1q, y1 = s * v1p + c * v1q;
    v1p = x1, v1q = y1;
    const double x2 = c * v2p - s * v2q, y2 = s * v2p + c * v2q;
    v2p = x2, v2q = y2;
}

__global__ __launch_bounds__(SEARCH_BLOCK) void cloud_normals_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                     const float4* __restrict__ sxyz, long n, int nx, int ny, int nz, double h,
                                                                     double up, float* __restrict__ normals, int* __restrict__ count,
                                                                     int* __restrict__ flatness, long long* __restrict__ sums) {
    __shared__ SearchTile tile;
    const long p = (long)blockIdx.x * SEARCH_BLOCK + threadIdx.x;
    const long long key = p < n ? keys[p] : CLOUD_DROPPED;
    const int cell = search_tile(tile, keys, p, key, keys, n, nx, ny, nz);   // the cloud is its own target
    long long k = 0, sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    if (key != CLOUD_DROPPED) {
        const float4 a = sxyz[p];
        const double cap2 = h * h;
        search_walk(tile, cell, sxyz, n, [&, a, cap2, h](int j, const float4 q) {
            if (!(cloud_d2(a, q) < cap2)) return;   // a NaN too
            const long long dx = llrint(((double)q.x - (double)a.x) / h * 1024.0), dy = llrint(((double)q.y - (double)a.y) / h * 1024.0),
                            dz = llrint(((double)q.z - (double)a.z) / h * 1024.0);
            k += 1;
            sx += dx, sy += dy, sz += dz;
            sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
        });
    }
    if (p >= n) return;   // (after the tile's barriers)
    const long long src = order[p];
    if (src < 0 || src >= n) return;   // never true for a sort order: a guard on the writes
    if (sums) {
        long long* s = sums + NORMALS_SUMS * src;
        s[0] = k, s[1] = sx, s[2] = sy, s[3] = sz, s[4] = sxx, s[5] = sxy, s[6] = sxz, s[7] = syy, s[8] = syz, s[9] = szz;
    }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    int flat = -1;
    if (k >= 3) {
        const double kk = (double)k, mx = (double)sx, my = (double)sy, mz = (double)sz;
        double axx = (double)sxx - (mx * mx) / kk, axy = (double)sxy - (mx * my) / kk, axz = (double)sxz - (mx * mz) / kk,
               ayy = (double)syy - (my * my) / kk, ayz = (double)syz - (my * mz) / kk, azz = (double)szz - (mz * mz) / kk;
        double vxx = 1.0, vxy = 0.0, vxz = 0.0, vyx = 0.0, vyy = 1.0, vyz = 0.0, vzx = 0.0, vzy = 0.0, vzz = 1.0;   // v[row][column]
#pragma unroll 1
        for (int sweep = 0; sweep < NORMALS_SWEEPS; ++sweep) {
            normals_rotate(axx, ayy, axy, axz, ayz, vxx, vxy, vyx, vyy, vzx, vzy);
            normals_rotate(axx, azz, axz, axy, ayz, vxx, vxz, vyx, vyz, vzx, vzz);
            normals_rotate(ayy, azz, ayz, axy, axz, vxy, vxz, vyy, vyz, vzy, vzz);
        }
        // the column of the smallest diagonal entry (the first of equal ones), by selects
        const bool x_least = axx <= ayy && axx <= azz, y_least = !x_least && ayy <= azz;
        const double l0 = x_least ? axx : (y_least ? ayy : azz), l2 = fmax(axx, fmax(ayy, azz)),
                     l1 = x_least ? fmin(ayy, azz) : (y_least ? fmin(axx, azz) : fmin(axx, ayy));
        if (l2 > 0.0 && l1 > 1e-12 * l2) {
            double ex = x_least ? vxx : (y_least ? vxy : vxz), ey = x_least ? vyx : (y_least ? vyy : vyz),
                   ez = x_least ? vzx : (y_least ? vzy : vzz);
            const double len = sqrt((ex * ex + ey * ey) + ez * ez);
            ex = ex / len, ey = ey / len, ez = ez / len;
            const double d = ez * up;
            const bool flip = d < 0.0 || (d == 0.0 && (ex < 0.0 || (ex == 0.0 && ey < 0.0)));
            n0 = flip ? -ex : ex, n1 = flip ? -ey : ey, n2 = flip ? -ez : ez;
            flat = (int)llrint(1024.0 * l0 / ((l0 + l1) + l2));
        }
    }
    normals[3 * src] = (float)n0, normals[3 * src + 1] = (float)n1, normals[3 * src + 2] = (float)n2;
    count[src] = (int)k;
    flatness[src] = flat;
}

}  // namespace d3d

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
using namespace d3d;

extern "C" size_t d3d_cloud_normals_scratch_bytes(long long n) {
    if (!count_ok(n)) return 0;
    return search_gather_bytes(n);
}

extern "C" int d3d_cloud_normals(const float* xyz, const long long* sorted_keys, const long long* order, long long n_points, int nx, int ny,
                                 int nz, double radius, int z_down, void* scratch, size_t scratch_bytes, float* normals, int* count,
                                 int* flatness, long long* sums_or_null, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_points), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE(scratch, "null pointer (scratch)");
    D3D_REQUIRE((xyz && sorted_keys && order && normals && count && flatness) || n_points == 0,
                "null pointer (xyz, sorted_keys, order, normals, count, flatness) with %lld points", n_points);
    if (search_grid_ok(nx, ny, nz, "cells") != D3D_OK) return D3D_ERR_INVALID_ARG;
    if (search_cap_ok(radius) != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(z_down == 0 || z_down == 1, "z_down=%d (0 or 1)", z_down);
    const size_t need = search_gather_bytes(n_points);
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_cloud_normals_scratch_bytes)", scratch_bytes, need);
    const size_t n = (size_t)n_points;
    const SearchRange R[8] = {{xyz, n * 12},    {sorted_keys, n * 8}, {order, n * 8},    {scratch, scratch_bytes},
                              {normals, n * 12}, {count, n * 4},       {flatness, n * 4}, {sums_or_null, n * NORMALS_SUMS * 8}};
    D3D_REQUIRE(search_apart(R, 8), "xyz, sorted_keys, order, scratch, normals, count, flatness and sums must not alias");
    if (n_points == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    float4* sxyz = (float4*)scratch;
    const int rc = search_gather(xyz, order, n_points, sxyz, st);
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(cloud_normals_kernel, dim3(ceil_div(n_points, SEARCH_BLOCK)), dim3(SEARCH_BLOCK), 0, st, sorted_keys, order, sxyz,
                       (long)n_points, nx, ny, nz, radius, z_down ? -1.0 : 1.0, normals, count, flatness, sums_or_null);
    D3D_LAUNCH_CHECK("cloud_normals_kernel launch");
    return D3D_OK;
}
