// The kernels behind geom_shared.h: the device-wide exclusive scan, the union-find passes and the compaction of kept faces.
#include "geom_shared.h"

namespace d3d {

constexpr int GEOM_BLOCK = 256, GEOM_SCAN_PER = GEOM_SCAN_TILE / GEOM_BLOCK;

// ---------------------------------------------------------------------------------------------------------------------------
// exclusive scan of int32 values: tile sums, one workgroup over the tile sums, then each tile with its offset
// ---------------------------------------------------------------------------------------------------------------------------
// The GEOM_SCAN_PER values of a lane, 0 past n: four 16-byte loads where the lane's run is whole and `in` is 16-byte aligned
// (the run starts at a multiple of 16 values).
__device__ __forceinline__ void geom_scan_load(const int* in, long base, long n, int* v) {
    if (base + GEOM_SCAN_PER <= n && ((uintptr_t)in & 15) == 0) {
        const int4* q = reinterpret_cast<const int4*>(in + base);
#pragma unroll
        for (int k = 0; k < GEOM_SCAN_PER / 4; ++k) {
            const int4 a = q[k];
            v[4 * k] = a.x, v[4 * k + 1] = a.y, v[4 * k + 2] = a.z, v[4 * k + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < GEOM_SCAN_PER; ++k) v[k] = base + k < n ? in[base + k] : 0;
    }
}

template <typename S>
__global__ __launch_bounds__(GEOM_BLOCK) void geom_scan_reduce_kernel(const int* __restrict__ in, long n, S* __restrict__ tile_sums) {
    __shared__ int lds[GEOM_BLOCK / 64];
    const long base = (long)blockIdx.x * GEOM_SCAN_TILE + (long)threadIdx.x * GEOM_SCAN_PER;
    int v[GEOM_SCAN_PER];
    geom_scan_load(in, base, n, v);
    int s = 0;
#pragma unroll
    for (int k = 0; k < GEOM_SCAN_PER; ++k) s += v[k];
    int total;
    block_exclusive<int>(s, lds, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

template <typename S>
__global__ __launch_bounds__(1024) void geom_scan_tiles_kernel(S* __restrict__ tile_sums, int n_tiles, long long* __restrict__ total) {
    __shared__ S lds[1024 / 64];
    S carry = 0;
    for (int base = 0; base < n_tiles; base += 1024) {
        const int i = base + threadIdx.x;
        const S x = i < n_tiles ? tile_sums[i] : 0;
        S all;
        const S ex = block_exclusive<S>(x, lds, &all);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

// out may be in: each lane reads its values before it writes them
template <typename S>
__global__ __launch_bounds__(GEOM_BLOCK) void geom_scan_apply_kernel(const int* in, long n, const S* __restrict__ tile_sums, int* out) {
    __shared__ int lds[GEOM_BLOCK / 64];
    const long base = (long)blockIdx.x * GEOM_SCAN_TILE + (long)threadIdx.x * GEOM_SCAN_PER;
    int v[GEOM_SCAN_PER];
    geom_scan_load(in, base, n, v);
    int s = 0;
#pragma unroll
    for (int k = 0; k < GEOM_SCAN_PER; ++k) s += v[k];
    int total;
    const int ex = block_exclusive<int>(s, lds, &total);
    S run = tile_sums[blockIdx.x] + ex;
#pragma unroll
    for (int k = 0; k < GEOM_SCAN_PER; ++k) {
        if (base + k < n) out[base + k] = (int)run;   // the totals decide whether these fit; the caller checks them
        run += v[k];
    }
}

template <typename S>
int geom_scan_sums(const int* in, int* out, long long n, S* sums, long long* total, hipStream_t st) {
    const long long tiles = geom_scan_tiles(n);
    if (tiles > 0) {
        hipLaunchKernelGGL(geom_scan_reduce_kernel<S>, dim3((unsigned)tiles), dim3(GEOM_BLOCK), 0, st, in, (long)n, sums);
        D3D_LAUNCH_CHECK("geom_scan_reduce_kernel launch");
    }
    hipLaunchKernelGGL(geom_scan_tiles_kernel<S>, dim3(1), dim3(1024), 0, st, sums, (int)tiles, total);
    D3D_LAUNCH_CHECK("geom_scan_tiles_kernel launch");
    if (tiles > 0) {
        hipLaunchKernelGGL(geom_scan_apply_kernel<S>, dim3((unsigned)tiles), dim3(GEOM_BLOCK), 0, st, in, (long)n, sums, out);
        D3D_LAUNCH_CHECK("geom_scan_apply_kernel launch");
    }
    return D3D_OK;
}

template int geom_scan_sums<long long>(const int*, int*, long long, long long*, long long*, hipStream_t);
template int geom_scan_sums<int>(const int*, int*, long long, int*, long long*, hipStream_t);

// ---------------------------------------------------------------------------------------------------------------------------
// union-find
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEOM_BLOCK) void geom_iota_kernel(int* __restrict__ parent, long long n) {
    const long v = (long)blockIdx.x * GEOM_BLOCK + threadIdx.x;
    if (v < n) parent[v] = (int)v;
}

__global__ __launch_bounds__(GEOM_BLOCK) void geom_jump_kernel(int* parent, long long n) {
    const long v = (long)blockIdx.x * GEOM_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int p0 = parent[v];
    int p = p0;
    for (int q = parent[p]; q != p; q = parent[p]) p = q;
    if (p != p0) parent[v] = p;
}

int geom_iota(int* parent, long long n, hipStream_t st) {
    if (n <= 0) return D3D_OK;
    hipLaunchKernelGGL(geom_iota_kernel, dim3(ceil_div(n, GEOM_BLOCK)), dim3(GEOM_BLOCK), 0, st, parent, n);
    D3D_LAUNCH_CHECK("geom_iota_kernel launch");
    return D3D_OK;
}

int geom_jump(int* parent, long long n, hipStream_t st) {
    if (n <= 0) return D3D_OK;
    hipLaunchKernelGGL(geom_jump_kernel, dim3(ceil_div(n, GEOM_BLOCK)), dim3(GEOM_BLOCK), 0, st, parent, n);
    D3D_LAUNCH_CHECK("geom_jump_kernel launch");
    return D3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// kept faces
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEOM_BLOCK) void geom_scatter_kept_kernel(const int* __restrict__ faces, long m, const int* __restrict__ remap,
                                                                       const int* __restrict__ keep, const int* __restrict__ pos,
                                                                       int* __restrict__ out_faces, int* __restrict__ referenced) {
    const long f = (long)blockIdx.x * GEOM_BLOCK + threadIdx.x;
    if (f >= m || !keep[f]) return;
    const long o = pos[f];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int v = faces[3 * f + e], x = remap ? remap[v] : v;
        out_faces[3 * o + e] = x;
        referenced[x] = 1;
    }
}

int geom_scatter_kept(const int* faces, long long m, const int* remap, void* scratch, const KeepScratch& L, int* out_faces,
                      int* referenced, long long* n_kept, hipStream_t st) {
    char* w = (char*)scratch;
    const int* keep = (const int*)(w + L.keep);
    int* pos = (int*)(w + L.pos);
    const int rc = geom_scan(keep, pos, m, w + L.scan, n_kept, st);
    if (rc != D3D_OK || m == 0) return rc;
    hipLaunchKernelGGL(geom_scatter_kept_kernel, dim3(ceil_div(m, GEOM_BLOCK)), dim3(GEOM_BLOCK), 0, st, faces, (long)m, remap, keep, pos,
                       out_faces, referenced);
    D3D_LAUNCH_CHECK("geom_scatter_kept_kernel launch");
    return D3D_OK;
}

}  // namespace d3d

extern "C" size_t d3d_mesh_scan_scratch_bytes(long long n) { return n < 0 ? 0 : d3d::geom_scan_bytes(n); }
