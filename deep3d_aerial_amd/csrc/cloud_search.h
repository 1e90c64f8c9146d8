// The cloud's grid of sorted 63-bit keys and the capped neighbour search on it, shared by the merge (cloud.hip),
// the outlier removal (cloud_outliers.hip, §4.28), the comparison of two clouds (cloud_compare.hip, §4.29) and the stages on top
// of them (§4.33 says what lives where): the key's constants, the lower bound in the sorted keys, the 18 bounds of a cell's 3 x 3 x 3 window, the tile
// of 256 sorted queries that shares those bounds in LDS, the walk over a cell's candidates, the gather that feeds it, d2 and e,
// and the host's checks of a grid, a cap and the buffers of a call.  Not part of the public ABI.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr long long CLOUD_AXIS_MAX = (1ll << 21) - 1;   // the largest n_a
constexpr long long CLOUD_DROPPED = LLONG_MAX;          // the key of an unkeyed point
constexpr int CLOUD_E_CAP = 1024;                       // e of a candidate at or past the cap, and of a missing one
constexpr int CLOUD_BOUNDS = 18;                        // 9 ranges, a first and a past-the-last sorted index each

// The first index in the sorted keys [lo, hi) whose key is >= k; hi when there is none.
__device__ __forceinline__ int cloud_lower(const long long* __restrict__ keys, int lo, int hi, long long k) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Bound b (0 .. 17) of the cell `key`, searched in [lo, hi): range r = b / 2 is row iy + r % 3 - 1 of layer iz + r / 3 - 1, cells
// ix - 1 .. ix + 1 clipped to the grid; an even b is its first sorted index, an odd b the index past its last.  A row outside the
// grid: `outside` (0 and 0 make an empty range).  The cell need not hold a key of `keys`: a range no key falls in is empty.
__device__ __forceinline__ int cloud_bound(const long long* __restrict__ keys, int lo, int hi, long long key, int b, int nx, int ny, int nz,
                                           int outside) {
    const int ix = (int)(key & CLOUD_AXIS_MAX), iy = (int)((key >> 21) & CLOUD_AXIS_MAX), iz = (int)(key >> 42);
    const int r = b >> 1;
    const int y = iy + r % 3 - 1, z = iz + r / 3 - 1;
    if (y < 0 || y >= ny || z < 0 || z >= nz) return outside;
    const long long row = ((long long)z << 42) | ((long long)y << 21);
    return cloud_lower(keys, lo, hi, (b & 1) ? (row | (long long)min(ix + 1, nx - 1)) + 1 : row | (long long)max(ix - 1, 0));
}

constexpr int SEARCH_BLOCK = 256;   // the lanes of a workgroup of the search: one tile of consecutive sorted queries, a lane each
constexpr int SEARCH_WAVES = SEARCH_BLOCK / 64;
constexpr int SEARCH_AHEAD = 4;     // candidates loaded ahead of their use

// What a tile keeps in LDS: the keys of its distinct query cells in key order, their bounds as [bound][cell] (consecutive cells
// on consecutive banks), the first and the last cell's bounds, and the scan's word per wave.
struct SearchTile {
    long long cell_key[SEARCH_BLOCK];
    int bound[CLOUD_BOUNDS][SEARCH_BLOCK];
    int edge[2][CLOUD_BOUNDS];
    int scan[SEARCH_WAVES];
};

// Fills `tile` for the SEARCH_BLOCK sorted queries of a workgroup and returns this lane's cell (>= 0 for a keyed lane).  q_keys:
// the queries' sorted keys, p this lane's sorted index and key its key (CLOUD_DROPPED past the end); t_keys: the nt sorted keys
// of the targets, which may be q_keys.  Every lane of the workgroup calls it; it ends on a barrier, after which every bound of
// every cell of the tile is in LDS.  A query cell need not hold a target: a range no target key falls in has equal ends.
__device__ __forceinline__ int search_tile(SearchTile& tile, const long long* __restrict__ q_keys, long p, long long key,
                                           const long long* __restrict__ t_keys, long nt, int nx, int ny, int nz) {
    const int tid = threadIdx.x;
    // the query cells of this tile, numbered in key order: a lane heads a cell when the lane before it holds another key
    const int head = key != CLOUD_DROPPED && (tid == 0 || q_keys[p - 1] != key) ? 1 : 0;
    int n_cells;
    const int cell = block_exclusive(head, tile.scan, &n_cells) + head - 1;   // >= 0 for a keyed lane: lane 0 heads a cell
    if (head) tile.cell_key[cell] = key;
    __syncthreads();
    // The key a bound searches for does not decrease from one query cell to the next (the cells are in key order, the row's
    // offset is the same and the clipping is monotone), so every cell's bound b lies between the first cell's and the last
    // cell's: those two are searched in all the target keys (from 0 for a first cell whose row is outside the grid, to nt for
    // such a last cell), the others between them, a few steps in keys this tile's points lie next to.
    if (tid < 2 * CLOUD_BOUNDS && n_cells > 0) {
        const int last = tid / CLOUD_BOUNDS, b = tid - CLOUD_BOUNDS * last;
        tile.edge[last][b] = cloud_bound(t_keys, 0, (int)nt, tile.cell_key[last ? n_cells - 1 : 0], b, nx, ny, nz, last ? (int)nt : 0);
    }
    __syncthreads();
    for (int t = tid; t < CLOUD_BOUNDS * n_cells; t += SEARCH_BLOCK) {
        const int c = t / CLOUD_BOUNDS, b = t - CLOUD_BOUNDS * c;
        tile.bound[b][c] = cloud_bound(t_keys, tile.edge[0][b], tile.edge[1][b], tile.cell_key[c], b, nx, ny, nz, 0);
    }
    __syncthreads();
    return cell;
}

// Hands every candidate of `cell` to use(j, record), j its sorted index in 0 .. nt - 1 and record = rec[j]: the 9 ranges in
// turn, SEARCH_AHEAD loads in flight before the first is used -- the lanes of a cell read the same addresses, one broadcast load
// a wave.
template <typename Use>
__device__ __forceinline__ void search_walk(const SearchTile& tile, int cell, const float4* __restrict__ rec, long nt, Use use) {
    for (int r = 0; r < 9; ++r) {
        const int j1 = min(tile.bound[2 * r + 1][cell], (int)nt);   // (never above nt: a guard on the loads)
        for (int j = max(tile.bound[2 * r][cell], 0); j < j1; j += SEARCH_AHEAD) {
            float4 q[SEARCH_AHEAD];
#pragma unroll
            for (int u = 0; u < SEARCH_AHEAD; ++u) q[u] = rec[min(j + u, j1 - 1)];
#pragma unroll
            for (int u = 0; u < SEARCH_AHEAD; ++u)
                if (j + u < j1) use(j + u, q[u]);
        }
    }
}

// rec[p] = {x, y, z, input index} of sorted point p, through the order: the candidates of a cell become consecutive 16-byte
// loads, and a tie rule on the input index needs no second load.  One launch of the family's one gather kernel (cloud.hip).
int search_gather(const float* xyz, const long long* order, long long n, float4* rec, hipStream_t st);

// The bytes of rec for n points (n >= 0).
inline size_t search_gather_bytes(long long n) { return align256((size_t)(n > 0 ? n : 1) * sizeof(float4)); }

// d2 of the pair (a, q): (dx dx + dy dy) + dz dz in fp64, each operation rounded once (the build sets -ffp-contract=off).
__device__ __forceinline__ double cloud_d2(const float4 a, const float4 q) {
    const double dx = (double)a.x - (double)q.x, dy = (double)a.y - (double)q.y, dz = (double)a.z - (double)q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// e of a pair with d2 < cap2 = h h.
__device__ __forceinline__ int cloud_e(double d2, double h) { return (int)min((long long)CLOUD_E_CAP, llrint(sqrt(d2) / h * 1024.0)); }

// A buffer of an entry point, for search_apart.
struct SearchRange {
    const void* p;
    size_t bytes;
};

// No two of the non-null, non-empty buffers overlap.
inline bool search_apart(const SearchRange* r, int n) {
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            if (!r[a].p || !r[b].p || !r[a].bytes || !r[b].bytes) continue;
            if (!geom_apart(r[a].p, r[a].bytes, r[b].p, r[b].bytes)) return false;
        }
    return true;
}

// The host's check of a grid's axis counts (`what`: "cells" or "voxels") and of a cap: D3D_OK, or the error set.
inline int search_grid_ok(int nx, int ny, int nz, const char* what) {
    D3D_REQUIRE(nx >= 1 && nx <= CLOUD_AXIS_MAX && ny >= 1 && ny <= CLOUD_AXIS_MAX && nz >= 1 && nz <= CLOUD_AXIS_MAX,
                "grid of %d x %d x %d %s (1 .. 2^21 - 1 per axis)", nx, ny, nz, what);
    return D3D_OK;
}

inline int search_cap_ok(double cap) {
    D3D_REQUIRE(std::isfinite(cap) && cap > 0.0, "cap %g must be finite and > 0", cap);
    return D3D_OK;
}

// The workgroups of a grid-stride kernel to launch: as many as the current device holds at once, so that the loop is balanced
// with every workgroup resident from the start, never more than `cap` (DESIGN.md §4.29 measured what a second round costs).  The
// occupancy query costs more than half a millisecond on the host, so its answer is kept per device in the caller's `known`
// (SEARCH_MAX_DEVICES zero-initialised ints, one array per kernel); two threads that race here store the same number.
constexpr int SEARCH_MAX_DEVICES = 64;

inline int search_resident(const void* kernel, int block, int cap, int* known, const char* what, int* out) {
    int dev = 0;
    int rc = hip_status(hipGetDevice(&dev), what);
    if (rc != D3D_OK) return rc;
    const bool slot = dev >= 0 && dev < SEARCH_MAX_DEVICES;
    if (slot && known[dev] > 0) {
        *out = known[dev];
        return D3D_OK;
    }
    int n_cu = 0, per_cu = 0;
    rc = hip_status(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev), what);
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0), what);
    if (rc != D3D_OK) return rc;
    long resident = (long)n_cu * per_cu;
    if (resident < 1) resident = 1;
    if (resident > cap) resident = cap;
    if (slot) known[dev] = (int)resident;
    *out = (int)resident;
    return D3D_OK;
}

}  // namespace d3d
