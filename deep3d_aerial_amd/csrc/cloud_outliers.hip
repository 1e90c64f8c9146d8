// Outlier removal on a point cloud by capped k-nearest-neighbour distances (deep3d_aerial_amd/cloud_outliers.py
// states the rule, include/deep3d_planesweep.h too, tests/test_cloud_outliers.py restates it in numpy).
//
// Grid: the cloud's (cloud.hip), one cell one radius h wide; a point is keyed by d3d_cloud_keys, the single copy of the keying
// rule.  A point it drops (key INT64_MAX) is unkeyed: D = -1, nn = -1, nobody's neighbour, not in the sums.
// Per keyed point i, over every other keyed point j (j != i by index, so a duplicate at distance 0 counts):
//   d2   = (dx dx + dy dy) + dz dz in fp64, dx = (double)x_i - (double)x_j, each operation rounded once (-ffp-contract=off)
//   cap2 = h h
//   e_ij = 1024 when d2 >= cap2, else min(1024, llrint(sqrt(d2) / h * 1024.0))
//   nn_i = the number of j with d2 < cap2
//   D_i  = the sum of the k smallest e_ij, a missing neighbour (fewer than k candidates) counting 1024
// A point within h lies in the 3 x 3 x 3 cells around i's cell and anything further adds exactly 1024, which is what a missing
// neighbour adds: the 27-cell window gives the unbounded k-nearest answer under the cap.  D_i is an integer in 0 .. 1024 k, so
// neither the order nor the tie-breaking of the selection can change it.
// Sums over the m keyed points, int64: sums[0] = m, sums[1] = S1 = sum D, sums[2] = S2 = sum D^2.  D <= 2^15 (k <= 32) and
// m < 2^31 keep S2 below 2^61.
//
// gather:    search_gather (cloud_search.h): the coordinates in key order as 16-byte records, so the candidates of a cell are
//            consecutive 16-byte loads.
// distances: one lane per sorted point, one workgroup per 256 consecutive sorted points.  ix is the key's low field, so the
//            candidates of a cell are 9 runs of up to three consecutive cells, each one pair of binary searches in the sorted
//            keys (cloud_bound: clipped to the grid, never reaching the next row).  The points of one cell share their 9
//            ranges: search_tile (cloud_search.h, which says why only the first and the last cell search all the keys) parks the
//            bounds of the workgroup's cells in LDS, the cloud's keys being both the queries and the targets.  Each lane then
//            streams the candidates of its cell's ranges (search_walk, four loads ahead of their use), skips itself, and keeps
//            the K smallest d2 in a sorted list of K fp64 registers (K = 8, 16 or 32 >= k, a template argument): an insertion
//            is K compare / select pairs at compile-time indices, so the list never leaves the registers (no scratch).  e does
//            not decrease with d2, so the e of the k smallest d2 are the k smallest e: the sqrt and the division run k times a
//            point, not once a candidate.  The list starts at cap2 everywhere: a candidate at or past the cap, or a missing one,
//            needs no insertion and counts 1024.  Results go back to input order through the order.
//            Built with -DD3D_CLOUD_OUTLIERS_PLAIN every lane runs its own 18 searches, takes e of every candidate within the
//            radius and keeps a list of k entries indexed at run time: the plain statement of the rule, the form
//            tools/cloud_outliers_bench.py --variant_library times beside this one.
// Sums:      per wave (shuffles), then per workgroup (LDS), then one integer atomicAdd per workgroup and sum, its result unused.
// Atomics: that integer atomicAdd, nothing else: the same bits for any input order.
// The lower bound, the 18-bound rule, the tile, the walk, the gather, d2 and e are cloud_search.h's, shared with cloud_compare.hip.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CO_K_MAX = 32;

// Inserts d into the increasing list c and drops the largest; every index is a compile-time constant after unrolling.
template <int K>
__device__ __forceinline__ void outl_insert(double (&c)[K], double d) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double lo = d < c[i] ? d : c[i];
        d = d < c[i] ? c[i] : d;
        c[i] = lo;
    }
}

// The sums of the workgroup into sums[0 .. 2]: m, S1, S2.
__device__ __forceinline__ void outl_sums(bool keyed, int dist, long long (*red)[SEARCH_WAVES], unsigned long long* __restrict__ sums) {
    const long long d = keyed ? (long long)dist : 0;
    const long long s0 = wave_sum<long long>(keyed ? 1 : 0), s1 = wave_sum(d), s2 = wave_sum(d * d);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = s0;
        red[1][w] = s1;
        red[2][w] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < SEARCH_WAVES; ++w) t += red[threadIdx.x][w];
        if (t != 0) atomicAdd(sums + threadIdx.x, (unsigned long long)t);
    }
}

// The results of sorted point p in input order; an unkeyed point gets -1 and -1.
__device__ __forceinline__ void outl_store(const long long* __restrict__ order, long p, long n, bool keyed, int dist, int nn,
                                           int* __restrict__ out_dist, int* __restrict__ out_nn) {
    if (p >= n) return;
    const long long src = order[p];
    if (src < 0 || src >= n) return;   // never true for a sort order: a guard on the writes
    out_dist[src] = keyed ? dist : -1;
    out_nn[src] = keyed ? nn : -1;
}

#ifndef D3D_CLOUD_OUTLIERS_PLAIN
template <int K>
__global__ __launch_bounds__(SEARCH_BLOCK) void cloud_outliers_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                      const float4* __restrict__ sxyz, long n, int nx, int ny, int nz,
                                                                      double h, int k, int* __restrict__ out_dist, int* __restrict__ out_nn,
                                                                      unsigned long long* __restrict__ sums) {
    __shared__ SearchTile tile;
    __shared__ long long red[3][SEARCH_WAVES];
    const long p = (long)blockIdx.x * SEARCH_BLOCK + threadIdx.x;
    const long long key = p < n ? keys[p] : CLOUD_DROPPED;
    const bool keyed = key != CLOUD_DROPPED;
    const int cell = search_tile(tile, keys, p, key, keys, n, nx, ny, nz);   // the cloud is its own target
    // e does not decrease with d2 (a correctly rounded sqrt, a division by h > 0, a product and llrint are monotone), so the k
    // smallest e are the e of the k smallest d2: the list holds d2, and the sqrt and the division run k times a point
    const double cap2 = h * h;
    double top[K];
#pragma unroll
    for (int i = 0; i < K; ++i) top[i] = cap2;
    int nn = 0;
    if (keyed) {
        const float4 a = sxyz[p];
        search_walk(tile, cell, sxyz, n, [&top, &nn, a, cap2, p](int j, const float4 q) {
            if (j == p) return;
            const double d2 = cloud_d2(a, q);
            nn += d2 < cap2 ? 1 : 0;                     // false for a NaN
            if (d2 < top[K - 1]) outl_insert(top, d2);   // top[K - 1] <= cap2
        });
    }
    int dist = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) dist += i < k ? (top[i] < cap2 ? cloud_e(top[i], h) : CLOUD_E_CAP) : 0;
    outl_store(order, p, n, keyed, dist, nn, out_dist, out_nn);
    outl_sums(keyed, dist, red, sums);
}
#else
__global__ __launch_bounds__(SEARCH_BLOCK) void cloud_outliers_plain_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                            const float4* __restrict__ sxyz, long n, int nx, int ny, int nz,
                                                                            double h, int k, int* __restrict__ out_dist,
                                                                            int* __restrict__ out_nn, unsigned long long* __restrict__ sums) {
    __shared__ long long red[3][SEARCH_WAVES];
    const long p = (long)blockIdx.x * SEARCH_BLOCK + threadIdx.x;
    const long long key = p < n ? keys[p] : CLOUD_DROPPED;
    const bool keyed = key != CLOUD_DROPPED;
    int top[CO_K_MAX];   // the k smallest so far, increasing; indexed at run time
    for (int i = 0; i < k; ++i) top[i] = CLOUD_E_CAP;
    int nn = 0;
    if (keyed) {
        const double cap2 = h * h;
        const float4 a = sxyz[p];
        for (int r = 0; r < 9; ++r) {
            const int j0 = cloud_bound(keys, 0, (int)n, key, 2 * r, nx, ny, nz, 0), j1 = cloud_bound(keys, 0, (int)n, key, 2 * r + 1, nx, ny, nz, 0);
            for (int j = j0; j < j1; ++j) {
                if (j == p) continue;
                const double d2 = cloud_d2(a, sxyz[j]);
                if (!(d2 < cap2)) continue;   // a NaN too
                nn += 1;
                const int e = cloud_e(d2, h);
                if (e >= top[k - 1]) continue;
                int i = k - 1;
                for (; i > 0 && top[i - 1] > e; --i) top[i] = top[i - 1];
                top[i] = e;
            }
        }
    }
    int dist = 0;
    for (int i = 0; i < k; ++i) dist += top[i];
    outl_store(order, p, n, keyed, dist, nn, out_dist, out_nn);
    outl_sums(keyed, dist, red, sums);
}
#endif

}  // namespace d3d

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
using namespace d3d;

extern "C" size_t d3d_cloud_outliers_scratch_bytes(long long n) {
    if (!count_ok(n)) return 0;
    return search_gather_bytes(n);
}

extern "C" int d3d_cloud_outliers_distances(const float* xyz, const long long* sorted_keys, const long long* order, long long n_points,
                                            int nx, int ny, int nz, double radius, int k, void* scratch, size_t scratch_bytes, int* dist,
                                            int* nn, long long* sums, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_points), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE(scratch && sums, "null pointer (scratch, sums)");
    D3D_REQUIRE((xyz && sorted_keys && order && dist && nn) || n_points == 0, "null pointer (xyz, sorted_keys, order, dist, nn) with %lld points",
                n_points);
    if (search_grid_ok(nx, ny, nz, "cells") != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(std::isfinite(radius) && radius > 0.0, "radius %g must be finite and > 0", radius);
    D3D_REQUIRE(k >= 1 && k <= CO_K_MAX, "k=%d (1 .. %d)", k, CO_K_MAX);
    const size_t need = search_gather_bytes(n_points);
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_cloud_outliers_scratch_bytes)", scratch_bytes, need);
    const size_t n = (size_t)n_points;
    const SearchRange R[7] = {{xyz, n * 12}, {sorted_keys, n * 8}, {order, n * 8}, {scratch, scratch_bytes}, {dist, n * 4}, {nn, n * 4}, {sums, 24}};
    D3D_REQUIRE(search_apart(R, 7), "xyz, sorted_keys, order, scratch, dist, nn and sums must not alias");
    if (n_points == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(sums, 0, 24, st), "cloud outliers: clear sums");
    if (rc != D3D_OK) return rc;
    const dim3 grid(ceil_div(n_points, SEARCH_BLOCK)), block(SEARCH_BLOCK);
    float4* sxyz = (float4*)scratch;
    const int rc2 = search_gather(xyz, order, n_points, sxyz, st);
    if (rc2 != D3D_OK) return rc2;
#ifndef D3D_CLOUD_OUTLIERS_PLAIN
#define CO_DISTANCES(K)                                                                                                               \
    hipLaunchKernelGGL((cloud_outliers_kernel<K>), grid, block, 0, st, sorted_keys, order, sxyz, (long)n_points, nx, ny, nz, radius, k, dist, nn, \
                       (unsigned long long*)sums)
    if (k <= 8) CO_DISTANCES(8);
    else if (k <= 16) CO_DISTANCES(16);
    else CO_DISTANCES(32);
#undef CO_DISTANCES
    D3D_LAUNCH_CHECK("cloud_outliers_kernel launch");
#else
    hipLaunchKernelGGL(cloud_outliers_plain_kernel, grid, block, 0, st, sorted_keys, order, sxyz, (long)n_points, nx, ny, nz, radius, k, dist, nn,
                       (unsigned long long*)sums);
    D3D_LAUNCH_CHECK("cloud_outliers_plain_kernel launch");
#endif
    return D3D_OK;
}
