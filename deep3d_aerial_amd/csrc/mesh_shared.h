// Helpers dsm.hip, mesh.hip and mesh_clean.hip share (not part of the public ABI).
#pragma once
#include "common.h"

namespace d3d {

// Order-preserving fp32 -> uint32 key: for non-NaN a, b, a < b exactly when dsm_key(a) < dsm_key(b), so integer atomicMin /
// atomicMax of keys give the float minimum / maximum whatever the order of the lanes.
__device__ __forceinline__ unsigned dsm_key(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float dsm_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Exclusive scan of one value per lane over the workgroup (blockDim.x a multiple of 64); *total gets the sum.
template <typename T>
__device__ __forceinline__ T mesh_block_exclusive(T x, T* lds, T* total) {
    // lds: one T per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    T inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
    for (int w = 0; w < n_waves; ++w) {
        const T v = lds[w];
        if (w < wave) before += v;
        all += v;
    }
    __syncthreads();
    *total = all;
    return before + inc - x;
}

// Exclusive scan of n int32 values into out (out may be in), *total (device int64) their sum; scratch of
// d3d_mesh_scan_scratch_bytes(n) bytes.  The caller checks that the total fits in int32.  mesh.hip.
int mesh_scan(const int* in, int* out, long long n, void* scratch, long long* total, hipStream_t st);

}  // namespace d3d
