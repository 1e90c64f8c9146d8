// Comparison of two point clouds by capped nearest-neighbour distances: accuracy, completeness, F-score (DESIGN.md §4.29;
// deep3d_aerial_amd/cloud_compare.py states the rule, include/deep3d_planesweep.h too, tests/test_cloud_compare.py restates it in
// numpy).
//
// Grid: the cloud's (cloud.hip), one cell one cap h wide; the queries Q and the targets T are both keyed by d3d_cloud_keys with
// voxel = h, the single copy of the keying rule.  A point it drops (key INT64_MAX) is unkeyed: as a query e = -1, idx = -1 and in
// no count; as a target nobody's neighbour.
// Per keyed query i, over every keyed target j:
//   d2   = (dx dx + dy dy) + dz dz in fp64, dx = (double)q_x - (double)t_x, each operation rounded once (-ffp-contract=off)
//   cap2 = h h
//   the nearest is the j with d2 < cap2 that minimises (d2, j), j the index in T's input order: of equally distant targets the
//   lowest input index wins
//   found:  idx_i = j, e_i = min(1024, llrint(sqrt(d2) / h * 1024.0))       (the outliers' e)
//   none:   idx_i = -1, e_i = 1024
// e does not decrease with d2, so e_i does not depend on the tie rule; idx_i does.  A target within h lies in the 3 x 3 x 3 cells
// around the query's cell: the 27-cell window is exact under the cap.
// hist [1026] int64, zeroed by the call: hist[e] (0 .. 1024) the keyed queries that found a neighbour with that e, hist[1025] the
// keyed queries that found none; sum(hist) = the keyed queries.
//
// gather:  search_gather (cloud_search.h): the targets in key order as 16-byte records {x, y, z, input index}: the candidates of
//          a cell are consecutive 16-byte loads and the tie rule needs no second load.
// nearest: the queries in THEIR key order, one lane each, 256 consecutive sorted queries a tile, the tiles dealt in a grid-stride
//          loop to as many workgroups as are resident at once (at most CC_GRID_CAP).  Per tile search_tile (cloud_search.h, which
//          says why only the first and the last cell search all the keys) parks the 18 bounds of the tile's distinct query cells,
//          searched in the TARGET's sorted keys, in LDS.  Each lane streams its 9 ranges (search_walk, four loads ahead) and keeps
//          one fp64 minimum and one index in registers; the sqrt and the division run once a query.  Results go back to input
//          order through the query's order.
// hist:    an unsigned [1026] histogram in LDS per workgroup, one LDS integer atomicAdd per keyed query, flushed once when the
//          workgroup has done all its tiles with one global integer atomicAdd per non-empty bin.
// Atomics: those two integer atomicAdd, results unused, nothing else: the same bits for any input order.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CC_BINS = 1026;        // e = 0 .. 1024, then the queries that found nothing
constexpr int CC_GRID_CAP = 2048;    // workgroups launched at most (fewer where fewer are resident); more tiles are looped over

__global__ __launch_bounds__(SEARCH_BLOCK) void cloud_compare_nearest_kernel(const float* __restrict__ q_xyz, const long long* __restrict__ q_keys,
                                                                         const long long* __restrict__ q_order, long nq,
                                                                         const long long* __restrict__ t_keys, const float4* __restrict__ t_rec,
                                                                         long nt, long n_tiles, int nx, int ny, int nz, double h,
                                                                         int* __restrict__ out_e, int* __restrict__ out_idx,
                                                                         unsigned long long* __restrict__ hist) {
    __shared__ SearchTile tile;
    __shared__ unsigned bins[CC_BINS];
    const int tid = threadIdx.x;
    for (int b = tid; b < CC_BINS; b += SEARCH_BLOCK) bins[b] = 0u;
    __syncthreads();
    const double cap2 = h * h;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {   // the same trip count for every lane of the workgroup
        const long p = t * SEARCH_BLOCK + tid;
        const long long key = p < nq ? q_keys[p] : CLOUD_DROPPED;
        const bool keyed = key != CLOUD_DROPPED;
        const int cell = search_tile(tile, q_keys, p, key, t_keys, nt, nx, ny, nz);
        long long src = -1;
        if (p < nq) {
            src = q_order[p];
            if (src < 0 || src >= nq) src = -1;   // never true for a sort order: a guard on the loads and the writes
        }
        double best = cap2;   // the smallest d2 below cap2 so far
        int best_j = -1;      // and the lowest input index that has it
        if (keyed && src >= 0) {
            const float4 a = make_float4(q_xyz[3 * src], q_xyz[3 * src + 1], q_xyz[3 * src + 2], 0.0f);
            search_walk(tile, cell, t_rec, nt, [&best, &best_j, a](int, const float4 q) {
                const double d2 = cloud_d2(a, q);
                const int jj = __float_as_int(q.w);
                // false for a NaN; best_j = -1 only while best = cap2, where the first comparison decides
                if (d2 < best || (d2 == best && jj < best_j)) {
                    best = d2;
                    best_j = jj;
                }
            });
        }
        const bool found = best_j >= 0;
        const int e = found ? cloud_e(best, h) : CLOUD_E_CAP;
        if (src >= 0) {
            out_e[src] = keyed ? e : -1;
            out_idx[src] = keyed ? best_j : -1;
        }
        if (keyed) atomicAdd(&bins[found ? e : CC_BINS - 1], 1u);
    }
    __syncthreads();
    for (int b = tid; b < CC_BINS; b += SEARCH_BLOCK) {
        const unsigned v = bins[b];
        if (v != 0u) atomicAdd(hist + b, (unsigned long long)v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
// The workgroups of the search to launch.  The tiles cost about the same, so the grid-stride loop is balanced when every workgroup
// is resident from the start: as many as the current device holds at once (24.2 KiB of LDS each: 6 a CU on gfx950, 1536), never
// more than CC_GRID_CAP.  With 2048 on 1536 slots the last quarter ran as a second round on a third of the chip (measured:
// DESIGN.md §4.29).  The query and its per-device cache are search_resident's (cloud_search.h).
static int cmp_resident(int* out) {
    static int known[SEARCH_MAX_DEVICES] = {};
    return search_resident((const void*)cloud_compare_nearest_kernel, SEARCH_BLOCK, CC_GRID_CAP, known, "cloud compare: resident workgroups", out);
}

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_cloud_compare_scratch_bytes(long long n_query, long long n_target) {
    if (!count_ok(n_query) || !count_ok(n_target)) return 0;
    return search_gather_bytes(n_target);
}

extern "C" int d3d_cloud_compare_nearest(const float* q_xyz, const long long* q_sorted_keys, const long long* q_order, long long n_query,
                                         const float* t_xyz, const long long* t_sorted_keys, const long long* t_order, long long n_target,
                                         int nx, int ny, int nz, double cap, void* scratch, size_t scratch_bytes, int* e, int* idx,
                                         long long* hist, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_query), "n_query=%lld (0 .. 2^31 - 1)", n_query);
    D3D_REQUIRE(count_ok(n_target), "n_target=%lld (0 .. 2^31 - 1)", n_target);
    D3D_REQUIRE(scratch && hist, "null pointer (scratch, hist)");
    D3D_REQUIRE((q_xyz && q_sorted_keys && q_order && e && idx) || n_query == 0,
                "null pointer (q_xyz, q_sorted_keys, q_order, e, idx) with %lld queries", n_query);
    D3D_REQUIRE((t_xyz && t_sorted_keys && t_order) || n_target == 0, "null pointer (t_xyz, t_sorted_keys, t_order) with %lld targets",
                n_target);
    if (search_grid_ok(nx, ny, nz, "cells") != D3D_OK || search_cap_ok(cap) != D3D_OK) return D3D_ERR_INVALID_ARG;
    const size_t need = search_gather_bytes(n_target);
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_cloud_compare_scratch_bytes)", scratch_bytes, need);
    const size_t nq = (size_t)n_query, nt = (size_t)n_target;
    const SearchRange R[10] = {{q_xyz, nq * 12}, {q_sorted_keys, nq * 8}, {q_order, nq * 8}, {t_xyz, nt * 12}, {t_sorted_keys, nt * 8},
                            {t_order, nt * 8}, {scratch, scratch_bytes}, {e, nq * 4}, {idx, nq * 4}, {hist, (size_t)CC_BINS * 8}};
    D3D_REQUIRE(search_apart(R, 10), "q_xyz, q_sorted_keys, q_order, t_xyz, t_sorted_keys, t_order, scratch, e, idx and hist must not alias");
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(hist, 0, (size_t)CC_BINS * 8, st), "cloud compare: clear hist");
    if (rc != D3D_OK) return rc;
    if (n_query == 0) return D3D_OK;
    float4* t_rec = (float4*)scratch;
    int resident = 0;
    int rc2 = search_gather(t_xyz, t_order, n_target, t_rec, st);
    if (rc2 == D3D_OK) rc2 = cmp_resident(&resident);
    if (rc2 != D3D_OK) return rc2;
    const long n_tiles = (long)((n_query + SEARCH_BLOCK - 1) / SEARCH_BLOCK);
    const dim3 grid((unsigned)(n_tiles < resident ? n_tiles : resident));
    hipLaunchKernelGGL(cloud_compare_nearest_kernel, grid, dim3(SEARCH_BLOCK), 0, st, q_xyz, q_sorted_keys, q_order, (long)n_query, t_sorted_keys,
                       (const float4*)t_rec, (long)n_target, n_tiles, nx, ny, nz, cap, e, idx, (unsigned long long*)hist);
    D3D_LAUNCH_CHECK("cloud_compare_nearest_kernel launch");
    return D3D_OK;
}
