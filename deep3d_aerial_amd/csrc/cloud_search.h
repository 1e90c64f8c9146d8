// The capped neighbour search on the cloud's one-radius grid of sorted 63-bit keys, shared by the outlier removal
// (cloud_outliers.hip) and the comparison of two clouds (cloud_compare.hip, §4.29): the lower bound in the sorted
// keys, the 18 bounds of a cell's 3 x 3 x 3 window, d2 and e, and the host's check that no two buffers of a call overlap.  Not
// part of the public ABI.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace d3d {

constexpr long long CLOUD_AXIS_MAX = (1ll << 21) - 1;   // the largest n_a (cloud.hip)
constexpr long long CLOUD_DROPPED = LLONG_MAX;          // the key of an unkeyed point (cloud.hip)
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
            const uintptr_t a0 = (uintptr_t)r[a].p, b0 = (uintptr_t)r[b].p;
            if (!(a0 + r[a].bytes <= b0 || b0 + r[b].bytes <= a0)) return false;
        }
    return true;
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
