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
// gather:  one lane per sorted target copies its coordinates and its input index through the order into a 16-byte record
//          {x, y, z, index} in key order: the candidates of a cell are consecutive 16-byte loads and the tie rule needs no second
//          load.
// nearest: the queries in THEIR key order, one lane each, 256 consecutive sorted queries a tile, the tiles dealt in a grid-stride
//          loop to as many workgroups as are resident at once (at most CC_GRID_CAP).  Per tile the workgroup numbers the distinct
//          query cells (a scan of the run heads), spreads their 18 bounds (cloud_search.h) over its lanes, searches them in the
//          TARGET's sorted keys and parks them in LDS ([bound][cell]).  The query cells are in key order, so a bound's key does
//          not decrease from cell to cell: only the first and the last cell search all the target keys, the others between those
//          two results.  A query cell need not hold a target: a range no target key falls in has equal ends and is empty.  Each
//          lane streams its 9 ranges four loads ahead -- the lanes of a cell read the same addresses -- and keeps one fp64 minimum
//          and one index in registers; the sqrt and the division run once a query.  Results go back to input order through the
//          query's order.
// hist:    an unsigned [1026] histogram in LDS per workgroup, one LDS integer atomicAdd per keyed query, flushed once when the
//          workgroup has done all its tiles with one global integer atomicAdd per non-empty bin.
// Atomics: those two integer atomicAdd, results unused, nothing else: the same bits for any input order.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CC_BLOCK = 256;
constexpr int CC_WAVES = CC_BLOCK / 64;
constexpr int CC_AHEAD = 4;          // candidates loaded ahead of their use
constexpr int CC_BINS = 1026;        // e = 0 .. 1024, then the queries that found nothing
constexpr int CC_GRID_CAP = 2048;    // workgroups launched at most (fewer where fewer are resident); more tiles are looped over

__global__ __launch_bounds__(CC_BLOCK) void cloud_compare_gather_kernel(const float* __restrict__ xyz, const long long* __restrict__ order,
                                                                        long n, float4* __restrict__ rec) {
    const long p = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const long long src = order[p];
    const bool ok = src >= 0 && src < n;   // always true for a sort order: a guard on the loads
    const float bad = __int_as_float(0x7fc00000);
    rec[p] = ok ? make_float4(xyz[3 * src], xyz[3 * src + 1], xyz[3 * src + 2], __int_as_float((int)src))
                : make_float4(bad, bad, bad, __int_as_float(-1));
}

__global__ __launch_bounds__(CC_BLOCK) void cloud_compare_nearest_kernel(const float* __restrict__ q_xyz, const long long* __restrict__ q_keys,
                                                                         const long long* __restrict__ q_order, long nq,
                                                                         const long long* __restrict__ t_keys, const float4* __restrict__ t_rec,
                                                                         long nt, long n_tiles, int nx, int ny, int nz, double h,
                                                                         int* __restrict__ out_e, int* __restrict__ out_idx,
                                                                         unsigned long long* __restrict__ hist) {
    __shared__ long long cell_key[CC_BLOCK];
    __shared__ int bound[CLOUD_BOUNDS][CC_BLOCK];
    __shared__ int edge[2][CLOUD_BOUNDS];
    __shared__ int scan_lds[CC_WAVES];
    __shared__ unsigned bins[CC_BINS];
    const int tid = threadIdx.x;
    for (int b = tid; b < CC_BINS; b += CC_BLOCK) bins[b] = 0u;
    __syncthreads();
    const double cap2 = h * h;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // the same trip count for every lane of the workgroup
        const long p = tile * CC_BLOCK + tid;
        const long long key = p < nq ? q_keys[p] : CLOUD_DROPPED;
        const bool keyed = key != CLOUD_DROPPED;
        // the query cells of this tile, numbered in key order: a lane heads a cell when the lane before it holds another key
        const int head = keyed && (tid == 0 || q_keys[p - 1] != key) ? 1 : 0;
        int n_cells;
        const int cell = block_exclusive(head, scan_lds, &n_cells) + head - 1;   // >= 0 for a keyed lane: lane 0 heads a cell
        if (head) cell_key[cell] = key;
        __syncthreads();
        // The key a bound searches for does not decrease from one query cell to the next (the cells are in key order, the row's
        // offset is the same and the clipping is monotone), so every cell's bound b lies between the first cell's and the last
        // cell's: those two are searched in all the target keys (from 0 for a first cell whose row is outside the grid, to nt for
        // such a last cell), the others between them.
        if (tid < 2 * CLOUD_BOUNDS && n_cells > 0) {
            const int last = tid / CLOUD_BOUNDS, b = tid - CLOUD_BOUNDS * last;
            edge[last][b] = cloud_bound(t_keys, 0, (int)nt, cell_key[last ? n_cells - 1 : 0], b, nx, ny, nz, last ? (int)nt : 0);
        }
        __syncthreads();
        for (int t = tid; t < CLOUD_BOUNDS * n_cells; t += CC_BLOCK) {
            const int c = t / CLOUD_BOUNDS, b = t - CLOUD_BOUNDS * c;
            bound[b][c] = cloud_bound(t_keys, edge[0][b], edge[1][b], cell_key[c], b, nx, ny, nz, 0);
        }
        __syncthreads();
        long long src = -1;
        if (p < nq) {
            src = q_order[p];
            if (src < 0 || src >= nq) src = -1;   // never true for a sort order: a guard on the loads and the writes
        }
        double best = cap2;   // the smallest d2 below cap2 so far
        int best_j = -1;      // and the lowest input index that has it
        if (keyed && src >= 0) {
            const float4 a = make_float4(q_xyz[3 * src], q_xyz[3 * src + 1], q_xyz[3 * src + 2], 0.0f);
            for (int r = 0; r < 9; ++r) {
                const int j1 = min(bound[2 * r + 1][cell], (int)nt);   // (never above nt: a guard on the loads)
                for (int j = max(bound[2 * r][cell], 0); j < j1; j += CC_AHEAD) {
                    float4 q[CC_AHEAD];   // CC_AHEAD loads in flight before the first is used
#pragma unroll
                    for (int u = 0; u < CC_AHEAD; ++u) q[u] = t_rec[min(j + u, j1 - 1)];
#pragma unroll
                    for (int u = 0; u < CC_AHEAD; ++u) {
                        if (j + u >= j1) continue;
                        const double d2 = cloud_d2(a, q[u]);
                        const int jj = __float_as_int(q[u].w);
                        // false for a NaN; best_j = -1 only while best = cap2, where the first comparison decides
                        if (d2 < best || (d2 == best && jj < best_j)) {
                            best = d2;
                            best_j = jj;
                        }
                    }
                }
            }
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
    for (int b = tid; b < CC_BINS; b += CC_BLOCK) {
        const unsigned v = bins[b];
        if (v != 0u) atomicAdd(hist + b, (unsigned long long)v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static bool cmp_count_ok(long long n) { return n >= 0 && n < (1ll << 31); }

static size_t cmp_scratch(long long n_target) { return align256((size_t)(n_target > 0 ? n_target : 1) * sizeof(float4)); }

// The workgroups of the search to launch.  The tiles cost about the same, so the grid-stride loop is balanced when every workgroup
// is resident from the start: as many as the current device holds at once (24.2 KiB of LDS each: 6 a CU on gfx950, 1536), never
// more than CC_GRID_CAP.  With 2048 on 1536 slots the last quarter ran as a second round on a third of the chip (measured:
// DESIGN.md §4.29).  The query and its per-device cache are search_resident's (cloud_search.h).
static int cmp_resident(int* out) {
    static int known[SEARCH_MAX_DEVICES] = {};
    return search_resident((const void*)cloud_compare_nearest_kernel, CC_BLOCK, CC_GRID_CAP, known, "cloud compare: resident workgroups", out);
}

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_cloud_compare_scratch_bytes(long long n_query, long long n_target) {
    if (!cmp_count_ok(n_query) || !cmp_count_ok(n_target)) return 0;
    return cmp_scratch(n_target);
}

extern "C" int d3d_cloud_compare_nearest(const float* q_xyz, const long long* q_sorted_keys, const long long* q_order, long long n_query,
                                         const float* t_xyz, const long long* t_sorted_keys, const long long* t_order, long long n_target,
                                         int nx, int ny, int nz, double cap, void* scratch, size_t scratch_bytes, int* e, int* idx,
                                         long long* hist, d3d_stream_t stream) {
    D3D_REQUIRE(cmp_count_ok(n_query), "n_query=%lld (0 .. 2^31 - 1)", n_query);
    D3D_REQUIRE(cmp_count_ok(n_target), "n_target=%lld (0 .. 2^31 - 1)", n_target);
    D3D_REQUIRE(scratch && hist, "null pointer (scratch, hist)");
    D3D_REQUIRE((q_xyz && q_sorted_keys && q_order && e && idx) || n_query == 0,
                "null pointer (q_xyz, q_sorted_keys, q_order, e, idx) with %lld queries", n_query);
    D3D_REQUIRE((t_xyz && t_sorted_keys && t_order) || n_target == 0, "null pointer (t_xyz, t_sorted_keys, t_order) with %lld targets",
                n_target);
    D3D_REQUIRE(nx >= 1 && nx <= CLOUD_AXIS_MAX && ny >= 1 && ny <= CLOUD_AXIS_MAX && nz >= 1 && nz <= CLOUD_AXIS_MAX,
                "grid of %d x %d x %d cells (1 .. 2^21 - 1 per axis)", nx, ny, nz);
    D3D_REQUIRE(std::isfinite(cap) && cap > 0.0, "cap %g must be finite and > 0", cap);
    const size_t need = cmp_scratch(n_target);
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
    if (n_target > 0) {
        hipLaunchKernelGGL(cloud_compare_gather_kernel, dim3(ceil_div(n_target, CC_BLOCK)), dim3(CC_BLOCK), 0, st, t_xyz, t_order, (long)n_target,
                           t_rec);
        D3D_LAUNCH_CHECK("cloud_compare_gather_kernel launch");
    }
    int resident = 0;
    const int rc2 = cmp_resident(&resident);
    if (rc2 != D3D_OK) return rc2;
    const long n_tiles = (long)((n_query + CC_BLOCK - 1) / CC_BLOCK);
    const dim3 grid((unsigned)(n_tiles < resident ? n_tiles : resident));
    hipLaunchKernelGGL(cloud_compare_nearest_kernel, grid, dim3(CC_BLOCK), 0, st, q_xyz, q_sorted_keys, q_order, (long)n_query, t_sorted_keys,
                       (const float4*)t_rec, (long)n_target, n_tiles, nx, ny, nz, cap, e, idx, (unsigned long long*)hist);
    D3D_LAUNCH_CHECK("cloud_compare_nearest_kernel launch");
    return D3D_OK;
}
