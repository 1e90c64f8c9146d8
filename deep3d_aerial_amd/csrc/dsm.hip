// Digital surface model from a point cloud: the reference's run.py:234-240 calls pc2dsm.DSM_from_PC, which it
// never shipped; the semantics are this project's (deep3d_aerial_amd/dsm.py states them, include/deep3d_planesweep.h too).
//
// Grid: cell (i, j) of point (x, y, z) is j = floor((x - x_min) / ux), i = floor((y_max - y) / uy) in fp64 with IEEE division;
// row 0 is north.  A point is kept when x, y, z are finite, 0 <= i < H, 0 <= j < W and z_min <= z <= z_max.
// Heights are compared through the order-preserving float -> uint32 key (IEEE total order, -0.0 < +0.0), so every selection is
// exact and does not depend on the order of the points.
//
// Max:        bin (one atomicAdd on count + one atomicMax of the key per point) -> finalize per cell.
// Robust_Max: bin (atomicAdd on count; the returned value is the point's rank in its cell, 4 B per point)
//             -> exclusive scan of count (the shared scan, geom_shared.h) -> scatter of the keys to offset[cell] + rank
//             -> select the (t+1)-th largest key, t = floor(trim * n): cells of up to DSM_SMALL points one lane each, keys
//                in registers; larger cells on a compacted list, one workgroup each, radix select over the key bytes with an
//                LDS histogram (a persistent grid walks the list: a cell of 10^5 points holds one workgroup, not the launch).
// MovingAverage: per empty cell, the mean of the non-empty cells of the (2r+1)^2 window (clipped to the raster), summed in
//             fp64 in the order dy = -r..r, dx = -r..r, divided by the count and rounded once; one launch per iteration.
// Every step is integer atomics or fixed-order arithmetic: the rasters are bit-reproducible for any point order or split.
// The DSM from a triangle mesh shares the grid, the key and the fill; its kernels follow the point kernels.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "dsm_tri.h"
#include "geom_shared.h"

namespace d3d {

constexpr int DSM_SMALL = 32;                               // cells of at most this many points: one lane, keys in registers
constexpr int DSM_BIG_GRID = 1024;                          // workgroups walking the list of larger cells
constexpr int DSM_FILL_TILE = 16;
constexpr int DSM_MAX_RADIUS = 16;

// The cell of point p, or -1.  Bin and scatter both call this, so they agree on every point.
__device__ __forceinline__ int dsm_cell(const float* __restrict__ xyz, long p, const DsmGrid& g, float* z_out) {
    const float x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
    *z_out = z;
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -1;
    const double zd = (double)z;
    if (!(zd >= g.z_min && zd <= g.z_max)) return -1;
    const double fj = floor(((double)x - g.x_min) / g.ux);
    const double fi = floor((g.y_max - (double)y) / g.uy);
    if (!(fj >= 0.0 && fj < (double)g.W && fi >= 0.0 && fi < (double)g.H)) return -1;
    return (int)fi * g.W + (int)fj;
}

template <bool ROBUST>
__global__ __launch_bounds__(DSM_BLOCK) void dsm_bin_kernel(const float* __restrict__ xyz, int n, DsmGrid g, int* __restrict__ count,
                                                            unsigned* __restrict__ keymax, int* __restrict__ rank) {
    const long p = (long)blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (p >= n) return;
    float z;
    const int c = dsm_cell(xyz, p, g, &z);
    if (c < 0) return;
    const int r = atomicAdd(count + c, 1);
    if constexpr (ROBUST)
        rank[p] = r;
    else
        atomicMax(keymax + c, dsm_key(z));
}

__global__ __launch_bounds__(DSM_BLOCK) void dsm_max_finalize_kernel(const int* __restrict__ count, const unsigned* __restrict__ keymax,
                                                                     int cells, int min_points, float* __restrict__ height) {
    const int c = blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const int n = count[c];
    height[c] = (n > 0 && n >= min_points) ? dsm_unkey(keymax[c]) : __builtin_nanf("");
}

__global__ __launch_bounds__(DSM_BLOCK) void dsm_scatter_kernel(const float* __restrict__ xyz, int n, DsmGrid g, const int* __restrict__ offset,
                                                                const int* __restrict__ rank, unsigned* __restrict__ keys) {
    const long p = (long)blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (p >= n) return;
    float z;
    const int c = dsm_cell(xyz, p, g, &z);
    if (c < 0) return;
    const int o = offset[c] + rank[p];
    if (o < n) keys[o] = dsm_key(z);   // always true (the scan counts what the bin kept): a guard on the write
}

__device__ __forceinline__ int dsm_trim_count(double trim, int n) { return (int)floor(trim * (double)n); }

// Cells of up to DSM_SMALL points: the keys in registers, the (t+1)-th largest found by walking down the distinct values
// (t + 1 <= n rounds at most; t = 0 -- every cell of fewer than 1 / trim points -- is one round, the plain maximum).
// Larger cells go on the list for dsm_select_big_kernel.
__global__ __launch_bounds__(DSM_BLOCK) void dsm_select_small_kernel(const int* __restrict__ count, const int* __restrict__ offset,
                                                                     const unsigned* __restrict__ keys, int cells, double trim,
                                                                     int min_points, float* __restrict__ height,
                                                                     int* __restrict__ big, int* __restrict__ n_big) {
    const int c = blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const int n = count[c];
    if (n == 0 || n < min_points) {
        height[c] = __builtin_nanf("");
        return;
    }
    if (n > DSM_SMALL) {
        big[atomicAdd(n_big, 1)] = c;
        return;
    }
    const unsigned* b = keys + offset[c];
    unsigned v[DSM_SMALL];
#pragma unroll
    for (int i = 0; i < DSM_SMALL; ++i) v[i] = i < n ? b[i] : 0u;   // valid keys are > 0: 0 is below every finite height
    int remaining = dsm_trim_count(trim, n) + 1;
    unsigned bound = 0xffffffffu, m = 0;
    bool first = true;
    for (;;) {
        m = 0;
        int eq = 0;
#pragma unroll
        for (int i = 0; i < DSM_SMALL; ++i) {
            const unsigned x = v[i];
            if (first || x < bound) {
                if (x > m) {
                    m = x;
                    eq = 1;
                } else if (x == m) {
                    ++eq;
                }
            }
        }
        if (eq >= remaining || m == 0) break;   // m == 0 cannot happen for t < n; it only guards the loop
        remaining -= eq;
        bound = m;
        first = false;
    }
    height[c] = dsm_unkey(m);
}

// One workgroup per listed cell: the key of rank t (descending) by four 8-bit radix passes, MSB first, LDS histogram.
__global__ __launch_bounds__(DSM_BLOCK) void dsm_select_big_kernel(const int* __restrict__ count, const int* __restrict__ offset,
                                                                   const unsigned* __restrict__ keys, const int* __restrict__ big,
                                                                   const int* __restrict__ n_big, double trim, float* __restrict__ height) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix;
    __shared__ int s_k;
    const int nb = *n_big;
    const int t = threadIdx.x;
    for (int q = blockIdx.x; q < nb; q += gridDim.x) {
        const int c = big[q];
        const int n = count[c];
        const unsigned* b = keys + offset[c];
        unsigned prefix = 0, mask = 0;
        int k = dsm_trim_count(trim, n);   // rank from the top, 0-based
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[t] = 0;
            __syncthreads();
            for (int i = t; i < n; i += DSM_BLOCK) {
                const unsigned x = b[i];
                if ((x & mask) == prefix) atomicAdd(hist + ((x >> shift) & 255u), 1u);
            }
            __syncthreads();
            if (t == 0) {
                int cum = 0;
                for (int d = 255; d >= 0; --d) {
                    const int h = (int)hist[d];
                    if (cum + h > k) {
                        s_k = k - cum;
                        s_prefix = prefix | ((unsigned)d << shift);
                        break;
                    }
                    cum += h;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            mask |= 255u << shift;
            __syncthreads();
        }
        if (t == 0) height[c] = dsm_unkey(prefix);
    }
}

// MovingAverage: a 16 x 16 tile of cells per workgroup, the tile and its halo of r in LDS (NaN outside the raster).
__global__ __launch_bounds__(DSM_FILL_TILE * DSM_FILL_TILE) void dsm_fill_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                                 int W, int H, int r) {
    constexpr int S = DSM_FILL_TILE + 2 * DSM_MAX_RADIUS;
    __shared__ float tile[S * S];
    const int side = DSM_FILL_TILE + 2 * r;
    const int x0 = blockIdx.x * DSM_FILL_TILE - r, y0 = blockIdx.y * DSM_FILL_TILE - r;
    const int tid = threadIdx.y * DSM_FILL_TILE + threadIdx.x;
    for (int idx = tid; idx < side * side; idx += DSM_FILL_TILE * DSM_FILL_TILE) {
        const int ly = idx / side, lx = idx - ly * side;
        const int gy = y0 + ly, gx = x0 + lx;
        tile[ly * S + lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? in[(long)gy * W + gx] : __builtin_nanf("");
    }
    __syncthreads();
    const int x = blockIdx.x * DSM_FILL_TILE + threadIdx.x, y = blockIdx.y * DSM_FILL_TILE + threadIdx.y;
    if (x >= W || y >= H) return;
    const float* ctr = tile + (threadIdx.y + r) * S + threadIdx.x + r;
    float v = *ctr;
    if (isnan(v)) {
        double sum = 0.0;
        int cnt = 0;
        for (int dy = -r; dy <= r; ++dy) {
            const float* row = ctr + dy * S;
            for (int dx = -r; dx <= r; ++dx) {
                const float a = row[dx];
                if (!isnan(a)) {
                    sum += (double)a;
                    ++cnt;
                }
            }
        }
        v = cnt > 0 ? (float)(sum / (double)cnt) : __builtin_nanf("");
    }
    out[(long)y * W + x] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// DSM from a triangle mesh (deep3d_aerial_amd/dsm.py states the semantics, tests/test_dsm_mesh.py restates them).
// The coverage primitives (DsmTri, dsm_tri_setup / _range / _sample) are in dsm_tri.h, shared with ortho_mesh.hip.
// A triangle's vertices are put in lexicographic (x, y, z) order (IEEE total order per component: the order of the weighted sum
// then depends on the triangle alone, not on its winding or first vertex).  Edge p -> q has endpoints (u, v) in lexicographic
// (x, y) order and s = +1 if (u, v) == (p, q), else -1; E(p, q, P) = s ((v.x - u.x)(P.y - u.y) - (v.y - u.y)(P.x - u.x)), fp64,
// no contraction: two triangles sharing an edge evaluate the same magnitudes on it (watertight).  D = E(a, b, c); 0 or
// non-finite D: no contribution.  w_a = sigma E(b, c, P), w_b = sigma E(c, a, P), w_c = sigma E(a, b, P), sigma = sign(D);
// the centre is covered when all w >= 0 and W = (w_a + w_b) + w_c > 0, and the sample is
// fp32(((w_a z_a + w_b z_b) + w_c z_c) / W), dropped outside [z_min, z_max].  A cell keeps the largest sample (atomicMax of
// dsm_key); cells with none are NaN.
//
// small: one lane per triangle tests the centres of its cell range (the XY box's centre range with a one-cell margin, clipped)
//        when that holds at most DSM_TRI_SMALL cells; larger ranges are appended to the big list (slot order does not matter:
//        every update is an integer max).
// big:   a persistent grid of DSM_TRI_GRID workgroups walks the list; chunk k (DSM_TRI_CHUNK consecutive cells of the range, row-major) of
//        listed triangle q belongs to workgroup (q + k) mod G.  A workgroup reads the list 256 entries at a time and skips the
//        entries with no chunk of its own, so a triangle over the whole raster costs ceil(W H / 256) chunks spread over every
//        workgroup (2900 x 2900: 32851 chunks, at most 33 per workgroup), and a list of many barely-big triangles costs each
//        workgroup one coalesced read per 256 entries plus its own chunks.  The grid is launched whole whatever the list holds
//        (the host does not read the list's length).
constexpr int DSM_TRI_SMALL = 64;      // cell ranges of at most this many cells: one lane, no list

__global__ __launch_bounds__(DSM_BLOCK) void dsm_tri_small_kernel(const float* __restrict__ vertices, int n_vertices,
                                                                  const int* __restrict__ faces, int n_faces, DsmGrid g,
                                                                  unsigned* __restrict__ keymax, int4* __restrict__ big,
                                                                  int* __restrict__ n_big) {
    const long f = (long)blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    DsmTri T;
    int j0, j1, i0, i1, corner[3];
    if (!dsm_tri_setup(vertices, n_vertices, faces, f, T, corner) || !dsm_tri_range(T, g, &j0, &j1, &i0, &i1)) return;
    const int nj = j1 - j0 + 1, ni = i1 - i0 + 1;
    if ((long)nj * ni > DSM_TRI_SMALL) {
        const int q = atomicAdd(n_big, 1);
        if (q < n_faces) big[q] = make_int4((int)f, i0 * g.W + j0, nj, ni);   // always true (one slot per face): a guard on the write
        return;
    }
    for (int i = i0; i <= i1; ++i)
        for (int j = j0; j <= j1; ++j) {
            float z;
            if (dsm_tri_sample(T, g, i, j, &z)) atomicMax(keymax + (long)i * g.W + j, dsm_key(z));
        }
}

__global__ __launch_bounds__(DSM_BLOCK) void dsm_tri_big_kernel(const float* __restrict__ vertices, int n_vertices,
                                                                const int* __restrict__ faces, int n_faces, DsmGrid g,
                                                                const int4* __restrict__ big, const int* __restrict__ n_big,
                                                                unsigned* __restrict__ keymax) {
    __shared__ int4 ent[DSM_BLOCK];
    __shared__ int first[DSM_BLOCK];
    const int nb = min(*n_big, n_faces);
    const int G = gridDim.x, b = blockIdx.x, t = threadIdx.x;
    for (int base = 0; base < nb; base += DSM_BLOCK) {
        const int q = base + t;
        int k0 = -1;
        if (q < nb) {
            const int4 e = big[q];
            ent[t] = e;
            const long chunks = ((long)e.z * e.w + DSM_TRI_CHUNK - 1) / DSM_TRI_CHUNK;
            const int k = dsm_tri_first_chunk(q, b, G);   // this workgroup's first chunk of entry q: (q + k) mod G == b
            k0 = k < chunks ? k : -1;
        }
        first[t] = k0;
        __syncthreads();
        const int m = min(DSM_BLOCK, nb - base);
        for (int e = 0; e < m; ++e) {
            const int k1 = first[e];   // uniform across the workgroup
            if (k1 < 0) continue;
            const int4 en = ent[e];
            DsmTri T;
            int corner[3];
            if (!dsm_tri_setup(vertices, n_vertices, faces, en.x, T, corner)) continue;   // listed faces passed it: a guard
            const int cells = en.z * en.w;
            const int j0 = en.y % g.W, i0 = en.y / g.W;
            for (long k = k1; k * DSM_TRI_CHUNK < cells; k += G)
                for (int u = 0; u < DSM_TRI_CHUNK; u += DSM_BLOCK) {
                    const long idx = k * DSM_TRI_CHUNK + u + t;
                    if (idx >= cells) break;
                    const int r = (int)(idx / en.z), c = (int)(idx - (long)r * en.z);
                    const int i = i0 + r, j = j0 + c;
                    float z;
                    if (i < g.H && j < g.W && dsm_tri_sample(T, g, i, j, &z)) atomicMax(keymax + (long)i * g.W + j, dsm_key(z));
                }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DSM_BLOCK) void dsm_key_finalize_kernel(const unsigned* __restrict__ keymax, int cells,
                                                                     float* __restrict__ height) {
    const int c = blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const unsigned k = keymax[c];
    height[c] = k ? dsm_unkey(k) : __builtin_nanf("");   // key 0 is the unkeyed NaN: no finite sample has it
}

struct DsmMeshScratch {
    size_t keymax, n_big, big, total;
};

static DsmMeshScratch dsm_mesh_layout(long long n_faces, long long cells) {
    ScratchLayout L;
    DsmMeshScratch s = {};
    s.keymax = L.take((size_t)cells * 4);
    s.n_big = L.take(4);
    s.big = L.take((size_t)n_faces * 16);
    s.total = L.bytes;
    return s;
}

struct DsmScratch {
    size_t keymax, rank, offset, partial, keys, big, n_big, total;
};

static DsmScratch dsm_layout(long long n, long long cells, int select) {
    ScratchLayout L;
    DsmScratch s = {};
    if (select == 0) {
        s.keymax = L.take((size_t)cells * 4);
    } else {
        s.rank = L.take((size_t)n * 4);
        s.offset = L.take((size_t)cells * 4);
        s.partial = L.take((size_t)geom_scan_tiles(cells) * 4);   // the scan's tile sums as int32
        s.keys = L.take((size_t)n * 4);
        s.big = L.take((size_t)std::min(cells, n / (DSM_SMALL + 1) + 1) * 4);
        s.n_big = L.take(4);
    }
    s.total = L.bytes;
    return s;
}

static bool dsm_dims_ok(long long n, int W, int H) {
    return n >= 0 && n < (1ll << 31) && W >= 1 && H >= 1 && (long long)W * H < (1ll << 31);
}

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_dsm_scratch_bytes(long long n_points, int W, int H, int select) {
    if (!dsm_dims_ok(n_points, W, H) || (select != 0 && select != 1)) return 0;
    return dsm_layout(n_points, (long long)W * H, select).total;
}

extern "C" int d3d_dsm_from_points(const float* xyz, long long n_points, double x_min, double y_max, double unit_x, double unit_y,
                                   double z_min, double z_max, int W, int H, int select, double trim, int min_points, void* scratch,
                                   size_t scratch_bytes, float* height, int* count, d3d_stream_t stream) {
    D3D_REQUIRE(height && count, "null pointer (height, count)");
    D3D_REQUIRE(xyz || n_points == 0, "null pointer (xyz) with %lld points", n_points);
    D3D_REQUIRE(n_points >= 0 && n_points < (1ll << 31), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "raster %d x %d: size must be >= 1 and W * H < 2^31", W, H);
    D3D_REQUIRE(std::isfinite(unit_x) && std::isfinite(unit_y) && unit_x > 0.0 && unit_y > 0.0, "unit (%g, %g) must be finite and > 0",
                unit_x, unit_y);
    D3D_REQUIRE(std::isfinite(x_min) && std::isfinite(y_max), "border (x_min %g, y_max %g) must be finite", x_min, y_max);
    D3D_REQUIRE(!std::isnan(z_min) && !std::isnan(z_max) && z_min <= z_max, "z bounds [%g, %g]", z_min, z_max);
    D3D_REQUIRE(select == 0 || select == 1, "select=%d (0 Max, 1 Robust_Max)", select);
    D3D_REQUIRE(trim >= 0.0 && trim < 1.0, "trim=%g outside [0, 1)", trim);
    D3D_REQUIRE(min_points >= 1, "min_points=%d (>= 1)", min_points);
    const long long cells = (long long)W * H;
    const DsmScratch L = dsm_layout(n_points, cells, select);
    D3D_REQUIRE(scratch || L.total == 0, "null pointer (scratch)");
    D3D_REQUIRE(scratch_bytes >= L.total, "scratch of %zu bytes, %zu needed (d3d_dsm_scratch_bytes)", scratch_bytes, L.total);
    const int n = (int)n_points, nc = (int)cells;
    const DsmGrid g = {x_min, y_max, unit_x, unit_y, z_min, z_max, W, H};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)scratch;
    int rc = hip_status(hipMemsetAsync(count, 0, (size_t)cells * 4, st), "dsm: clear count");
    if (rc != D3D_OK) return rc;
    const int gp = ceil_div(n, DSM_BLOCK), gc = ceil_div(nc, DSM_BLOCK);
    if (select == 0) {
        unsigned* keymax = (unsigned*)(s + L.keymax);
        rc = hip_status(hipMemsetAsync(keymax, 0, (size_t)cells * 4, st), "dsm: clear keys");
        if (rc != D3D_OK) return rc;
        if (n > 0) {
            hipLaunchKernelGGL((dsm_bin_kernel<false>), dim3(gp), dim3(DSM_BLOCK), 0, st, xyz, n, g, count, keymax, (int*)nullptr);
            D3D_LAUNCH_CHECK("dsm_bin_kernel launch");
        }
        hipLaunchKernelGGL(dsm_max_finalize_kernel, dim3(gc), dim3(DSM_BLOCK), 0, st, count, keymax, nc, min_points, height);
        D3D_LAUNCH_CHECK("dsm_max_finalize_kernel launch");
        return D3D_OK;
    }
    int* rank = (int*)(s + L.rank);
    int* offset = (int*)(s + L.offset);
    int* partial = (int*)(s + L.partial);
    unsigned* keys = (unsigned*)(s + L.keys);
    int* big = (int*)(s + L.big);
    int* n_big = (int*)(s + L.n_big);
    rc = hip_status(hipMemsetAsync(n_big, 0, 4, st), "dsm: clear list");
    if (rc != D3D_OK) return rc;
    if (n > 0) {
        hipLaunchKernelGGL((dsm_bin_kernel<true>), dim3(gp), dim3(DSM_BLOCK), 0, st, xyz, n, g, count, (unsigned*)nullptr, rank);
        D3D_LAUNCH_CHECK("dsm_bin_kernel launch");
        rc = geom_scan_sums<int>(count, offset, cells, partial, nullptr, st);   // the total is at most n_points < 2^31
        if (rc != D3D_OK) return rc;
        hipLaunchKernelGGL(dsm_scatter_kernel, dim3(gp), dim3(DSM_BLOCK), 0, st, xyz, n, g, offset, rank, keys);
        D3D_LAUNCH_CHECK("dsm_scatter_kernel launch");
    } else {
        // no point: every count is 0, the select kernel reads neither offset nor keys
    }
    hipLaunchKernelGGL(dsm_select_small_kernel, dim3(gc), dim3(DSM_BLOCK), 0, st, count, offset, keys, nc, trim, min_points, height, big,
                       n_big);
    D3D_LAUNCH_CHECK("dsm_select_small_kernel launch");
    if (n > DSM_SMALL) {
        const long long cap = std::min(cells, n_points / (DSM_SMALL + 1) + 1);
        const int grid = (int)std::min<long long>(cap, DSM_BIG_GRID);
        hipLaunchKernelGGL(dsm_select_big_kernel, dim3(grid), dim3(DSM_BLOCK), 0, st, count, offset, keys, big, n_big, trim, height);
        D3D_LAUNCH_CHECK("dsm_select_big_kernel launch");
    }
    return D3D_OK;
}

extern "C" int d3d_dsm_fill_moving_average(const float* in, float* out, int W, int H, int radius, d3d_stream_t stream) {
    D3D_REQUIRE(in && out, "null pointer (in, out)");
    D3D_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "raster %d x %d: size must be >= 1 and W * H < 2^31", W, H);
    D3D_REQUIRE(radius >= 1 && radius <= DSM_MAX_RADIUS, "radius=%d outside 1..%d", radius, DSM_MAX_RADIUS);
    const size_t bytes = (size_t)W * H * 4;
    D3D_REQUIRE((uintptr_t)in + bytes <= (uintptr_t)out || (uintptr_t)out + bytes <= (uintptr_t)in,
                "out must not alias in (one launch per iteration ping-pongs two rasters)");
    const dim3 grid(ceil_div(W, DSM_FILL_TILE), ceil_div(H, DSM_FILL_TILE)), block(DSM_FILL_TILE, DSM_FILL_TILE);
    D3D_REQUIRE(grid.y <= 65535, "H=%d too large", H);
    hipLaunchKernelGGL(dsm_fill_kernel, grid, block, 0, (hipStream_t)stream, in, out, W, H, radius);
    D3D_LAUNCH_CHECK("dsm_fill_kernel launch");
    return D3D_OK;
}

extern "C" size_t d3d_dsm_mesh_scratch_bytes(long long n_faces, int W, int H) {
    if (!dsm_dims_ok(n_faces, W, H)) return 0;
    return dsm_mesh_layout(n_faces, (long long)W * H).total;
}

extern "C" int d3d_dsm_from_mesh(const float* vertices, long long n_vertices, const int* faces, long long n_faces, double x_min,
                                 double y_max, double unit_x, double unit_y, double z_min, double z_max, int W, int H, void* scratch,
                                 size_t scratch_bytes, float* height, d3d_stream_t stream) {
    D3D_REQUIRE(height && scratch, "null pointer (height, scratch)");
    D3D_REQUIRE(vertices || n_vertices == 0, "null pointer (vertices) with %lld vertices", n_vertices);
    D3D_REQUIRE(faces || n_faces == 0, "null pointer (faces) with %lld faces", n_faces);
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    D3D_REQUIRE(n_faces >= 0 && n_faces < (1ll << 31), "n_faces=%lld (0 .. 2^31 - 1)", n_faces);
    D3D_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "raster %d x %d: size must be >= 1 and W * H < 2^31", W, H);
    D3D_REQUIRE(std::isfinite(unit_x) && std::isfinite(unit_y) && unit_x > 0.0 && unit_y > 0.0, "unit (%g, %g) must be finite and > 0",
                unit_x, unit_y);
    D3D_REQUIRE(std::isfinite(x_min) && std::isfinite(y_max), "border (x_min %g, y_max %g) must be finite", x_min, y_max);
    D3D_REQUIRE(!std::isnan(z_min) && !std::isnan(z_max) && z_min <= z_max, "z bounds [%g, %g]", z_min, z_max);
    const long long cells = (long long)W * H;
    const DsmMeshScratch L = dsm_mesh_layout(n_faces, cells);
    D3D_REQUIRE(scratch_bytes >= L.total, "scratch of %zu bytes, %zu needed (d3d_dsm_mesh_scratch_bytes)", scratch_bytes, L.total);
    const uintptr_t h0 = (uintptr_t)height, h1 = h0 + (size_t)cells * 4, s0 = (uintptr_t)scratch, s1 = s0 + scratch_bytes;
    D3D_REQUIRE(h1 <= s0 || s1 <= h0, "height must not alias scratch");
    const int nf = (int)n_faces, nc = (int)cells;
    const DsmGrid g = {x_min, y_max, unit_x, unit_y, z_min, z_max, W, H};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)scratch;
    unsigned* keymax = (unsigned*)(s + L.keymax);
    int* n_big = (int*)(s + L.n_big);
    int4* big = (int4*)(s + L.big);
    int rc = hip_status(hipMemsetAsync(keymax, 0, (size_t)cells * 4, st), "dsm mesh: clear keys");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(n_big, 0, 4, st), "dsm mesh: clear list");
    if (rc != D3D_OK) return rc;
    if (nf > 0) {
        hipLaunchKernelGGL(dsm_tri_small_kernel, dim3(ceil_div(nf, DSM_BLOCK)), dim3(DSM_BLOCK), 0, st, vertices, (int)n_vertices, faces, nf,
                           g, keymax, big, n_big);
        D3D_LAUNCH_CHECK("dsm_tri_small_kernel launch");
        hipLaunchKernelGGL(dsm_tri_big_kernel, dim3(DSM_TRI_GRID), dim3(DSM_BLOCK), 0, st, vertices, (int)n_vertices, faces,
                           nf, g, big, n_big, keymax);
        D3D_LAUNCH_CHECK("dsm_tri_big_kernel launch");
    }
    hipLaunchKernelGGL(dsm_key_finalize_kernel, dim3(ceil_div(nc, DSM_BLOCK)), dim3(DSM_BLOCK), 0, st, keymax, nc, height);
    D3D_LAUNCH_CHECK("dsm_key_finalize_kernel launch");
    return D3D_OK;
}
