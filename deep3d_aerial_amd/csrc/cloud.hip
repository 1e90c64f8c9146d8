// Voxel-grid merge of the fused points into one de-duplicated cloud (deep3d_aerial_amd/cloud.py states the rule,
// include/deep3d_planesweep.h too, tests/test_cloud.py restates it in numpy).
//
// Grid: border = [Xmin, Xmax, Ymin, Ymax, Zmin, Zmax], voxel v, n_a = ceil((max_a - min_a) / v) in 1 .. 2^21 - 1 per axis.
// Cell of a point, per axis: u = ((double)x - min_a) / v, i = floor(u), r = floor((u - i) * 65536) in 0 .. 65535.  A point with a
// non-finite coordinate or an i outside 0 .. n_a - 1 is dropped (a point on a max face whose u equals n_a too) and gets the key
// INT64_MAX; every other point gets (iz << 42) | (iy << 21) | ix.
// Per occupied voxel, integer sums over its members: count; S_a = sum r_a; with normals N_c = sum llrint(n_c * 2^20) over the
// members whose normal is finite with every |n_c| <= 1024 (the others add nothing); with colours C_c = sum clamp(c, 0, 255).
//   position   min_a + (i_a + (S_a + 0.5 count) / (65536.0 count)) * v in fp64, each operation rounded once, then fp32
//   normal     N / |N| in fp64, |N| = sqrt((N_x N_x + N_y N_y) + N_z N_z), then fp32; (0, 0, 0) when N is zero
//   colour     (2 C_c + count) / (2 count) in integers (.5 rounds up), uint8
// A voxel is kept when the counts of its 3 x 3 x 3 neighbourhood (itself included, neighbours outside the grid do not exist) sum
// to at least min_points, over the unfiltered set, once.  The kept voxels come out in increasing key.
//
// No product feeds an addition unrounded: the library is built with -ffp-contract=off (the Makefile's CXXFLAGS), which is how
// dsm_tri.h keeps its fp64 chains uncontracted, so `a + b * c` below is a multiplication and an addition, as in numpy.
//
// keys:       one lane per point: the key and the three r packed into one int64 (r_x | r_y << 16 | r_z << 32).
// (sort)      torch.sort of the keys on the Python side: sorted keys and the order.
// heads:      one lane per sorted point marks the point that ends a run of equal keys (the next key differs: the head of the
//             next run follows it), not for the dropped keys; geom_scan's exclusive scan of the marks is then the voxel index of
//             every sorted point, and its total the number of voxels.
// accumulate: one lane per sorted point reads its point through the order and adds into its voxel's accumulators.  The keys are
//             sorted, so the lanes of a wave hold few runs: the run reduction of geom_shared.h (wave_run_sum; legal because
//             every sum is an integer) leaves each run's sum in its last lane, which issues the atomics and stores the voxel's
//             key.  A run that crosses waves adds once per wave.  Built with -DD3D_CLOUD_PLAIN every lane issues its own atomics
//             instead: the form tools/cloud_bench.py --variant_library times beside this one.
// neighbours: one lane per voxel.  ix is the low field of the key, so the 27 neighbours are 9 runs of up to three consecutive
//             keys, each one pair of binary searches in the unique keys (cloud_lower, cloud_search.h) and one difference of the
//             exclusive scan of the counts.  A run is clipped to 0 .. n_x - 1 and rows and layers outside the grid are skipped:
//             it never reaches the next row (the window of cloud_bound).
// gather:     not a step of the merge: the kernel behind search_gather (cloud_search.h), kept here so that the library holds it once.
// finalize:   the scan of the keep flags places the kept voxels; one lane per voxel writes its outputs.
// Atomics: integer atomicAdd with the result unused, nothing else: the same bits for any input order.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CL_BLOCK = 256;
constexpr float CL_NORMAL_MAX = 1024.0f;                       // |n_c| above this adds nothing: 2^31 members cannot overflow int64

struct CloudGrid {
    double lo[3], v;
    int n[3];
};

// i and r of one coordinate; false when the point is dropped
__device__ __forceinline__ bool cloud_cell(float x, double lo, double v, int n, long long* i, long long* r) {
    const double u = ((double)x - lo) / v;
    const double fi = floor(u);
    if (!(isfinite(x) && fi >= 0.0 && fi <= (double)(n - 1))) return false;
    *i = (long long)fi;
    *r = (long long)floor((u - fi) * 65536.0);
    return true;
}

__global__ __launch_bounds__(CL_BLOCK) void cloud_keys_kernel(const float* __restrict__ xyz, long n, CloudGrid g,
                                                              long long* __restrict__ keys, long long* __restrict__ frac) {
    const long p = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    long long i[3], r[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = cloud_cell(xyz[3 * p + a], g.lo[a], g.v, g.n[a], i + a, r + a) && ok;
    keys[p] = ok ? (i[2] << 42) | (i[1] << 21) | i[0] : CLOUD_DROPPED;
    frac[p] = ok ? r[0] | (r[1] << 16) | (r[2] << 32) : 0;
}

// search_gather (cloud_search.h): the family's one gather, for the searches of cloud_outliers.hip and cloud_compare.hip.
__global__ __launch_bounds__(CL_BLOCK) void cloud_gather_kernel(const float* __restrict__ xyz, const long long* __restrict__ order, long n,
                                                                float4* __restrict__ rec) {
    const long p = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const long long src = order[p];
    const bool ok = src >= 0 && src < n;   // always true for a sort order: a guard on the loads
    const float bad = __int_as_float(0x7fc00000);
    rec[p] = ok ? make_float4(xyz[3 * src], xyz[3 * src + 1], xyz[3 * src + 2], __int_as_float((int)src))
                : make_float4(bad, bad, bad, __int_as_float(-1));
}

int search_gather(const float* xyz, const long long* order, long long n, float4* rec, hipStream_t st) {
    if (n <= 0) return D3D_OK;
    hipLaunchKernelGGL(cloud_gather_kernel, dim3(ceil_div(n, CL_BLOCK)), dim3(CL_BLOCK), 0, st, xyz, order, (long)n, rec);
    D3D_LAUNCH_CHECK("cloud_gather_kernel launch");
    return D3D_OK;
}

__global__ __launch_bounds__(CL_BLOCK) void cloud_heads_kernel(const long long* __restrict__ keys, long n, int* __restrict__ mark) {
    const long p = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const long long k = keys[p];
    mark[p] = k != CLOUD_DROPPED && (p + 1 == n || keys[p + 1] != k) ? 1 : 0;
}

__device__ __forceinline__ void cloud_add(long long* p, long long x) { atomicAdd((unsigned long long*)p, (unsigned long long)x); }

// acc [n_voxels, stride] int64: S at 0, N at 3 (with normals), C after them (with colours)
template <bool NRM, bool COL>
__global__ __launch_bounds__(CL_BLOCK) void cloud_accumulate_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                                    const int* __restrict__ vox, const long long* __restrict__ frac,
                                                                    const float* __restrict__ normal, const int* __restrict__ color, long n,
                                                                    int n_voxels, long long* __restrict__ ukeys, int* __restrict__ count,
                                                                    long long* __restrict__ acc) {
    constexpr int STRIDE = 3 + (NRM ? 3 : 0) + (COL ? 3 : 0);
    const long p = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    const long long key = p < n ? keys[p] : CLOUD_DROPPED;
    int v = key != CLOUD_DROPPED ? vox[p] : -1;
    if (v >= n_voxels) v = -1;   // never true (the scan's total is n_voxels): a guard on the writes
    int c = 0, r[3] = {0, 0, 0}, col[3] = {0, 0, 0};
    long long nq[3] = {0, 0, 0};
    if (v >= 0) {
        const long long src = order[p];
        if (src >= 0 && src < n) {   // always true for a sort order: a guard on the loads
            c = 1;
            const long long f = frac[src];
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = (int)((f >> (16 * a)) & 0xffff);
            if (NRM) {
                const float nx = normal[3 * src], ny = normal[3 * src + 1], nz = normal[3 * src + 2];
                if (fabsf(nx) <= CL_NORMAL_MAX && fabsf(ny) <= CL_NORMAL_MAX && fabsf(nz) <= CL_NORMAL_MAX) {   // false for a NaN
                    nq[0] = llrint((double)nx * 1048576.0);
                    nq[1] = llrint((double)ny * 1048576.0);
                    nq[2] = llrint((double)nz * 1048576.0);
                }
            }
            if (COL) {
#pragma unroll
                for (int a = 0; a < 3; ++a) col[a] = min(max(color[3 * src + a], 0), 255);
            }
        } else {
            v = -1;
        }
    }
#ifndef D3D_CLOUD_PLAIN
    const int lane = threadIdx.x & 63;
    // 64 lanes of at most 65535 or 255 each: the sums of a wave fit in int32
    const int first = wave_run_first(v, lane);
    c = wave_run_sum(c, first, lane);
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = wave_run_sum(r[a], first, lane);
    if (NRM) {
#pragma unroll
        for (int a = 0; a < 3; ++a) nq[a] = wave_run_sum(nq[a], first, lane);
    }
    if (COL) {
#pragma unroll
        for (int a = 0; a < 3; ++a) col[a] = wave_run_sum(col[a], first, lane);
    }
    if (!wave_run_last(v, lane)) return;   // not the last lane of its run in this wave
#endif
    if (v < 0) return;
    ukeys[v] = key;   // every lane that gets here for v stores the same key
    atomicAdd(count + v, c);
    long long* A = acc + (long)v * STRIDE;
#pragma unroll
    for (int a = 0; a < 3; ++a) cloud_add(A + a, (long long)r[a]);
    if (NRM) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (nq[a] != 0) cloud_add(A + 3 + a, nq[a]);
    }
    if (COL) {
#pragma unroll
        for (int a = 0; a < 3; ++a) cloud_add(A + (NRM ? 6 : 3) + a, (long long)col[a]);
    }
}

__global__ __launch_bounds__(CL_BLOCK) void cloud_neighbours_kernel(const long long* __restrict__ ukeys, const int* __restrict__ count,
                                                                    const int* __restrict__ before, int n_voxels, int nx, int ny, int nz,
                                                                    int min_points, int* __restrict__ keep) {
    const int v = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (v >= n_voxels) return;
    if (min_points <= 1) {   // every voxel has a member
        keep[v] = 1;
        return;
    }
    const long long key = ukeys[v];
    // The window of cloud_bound (cloud_search.h), written as loops over the rows and layers inside the grid: stated with
    // cloud_bound itself the kernel was 0.5 % slower at 10^8 points.
    const int ix = (int)(key & CLOUD_AXIS_MAX), iy = (int)((key >> 21) & CLOUD_AXIS_MAX), iz = (int)(key >> 42);
    const int x0 = max(ix - 1, 0), x1 = min(ix + 1, nx - 1);
    long long sum = 0;
    for (int z = max(iz - 1, 0); z <= min(iz + 1, nz - 1); ++z)
        for (int y = max(iy - 1, 0); y <= min(iy + 1, ny - 1); ++y) {
            const long long row = ((long long)z << 42) | ((long long)y << 21);
            const int a = cloud_lower(ukeys, 0, n_voxels, row | x0), b = cloud_lower(ukeys, 0, n_voxels, (row | x1) + 1);
            if (b > a) sum += (long long)before[b - 1] + count[b - 1] - before[a];
        }
    keep[v] = sum >= (long long)min_points ? 1 : 0;
}

template <bool NRM, bool COL>
__global__ __launch_bounds__(CL_BLOCK) void cloud_finalize_kernel(const long long* __restrict__ ukeys, const int* __restrict__ count,
                                                                  const long long* __restrict__ acc, const int* __restrict__ keep,
                                                                  const int* __restrict__ pos, int n_voxels, int n_kept, CloudGrid g,
                                                                  float* __restrict__ xyz, float* __restrict__ normal,
                                                                  unsigned char* __restrict__ color, int* __restrict__ out_count) {
    constexpr int STRIDE = 3 + (NRM ? 3 : 0) + (COL ? 3 : 0);
    const int v = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (v >= n_voxels || !keep[v]) return;
    const long o = pos[v];
    if (o >= n_kept) return;   // never true (n_kept is the scan's total): a guard on the writes
    const long long key = ukeys[v];
    const long long i[3] = {key & CLOUD_AXIS_MAX, (key >> 21) & CLOUD_AXIS_MAX, key >> 42};
    const int c = count[v];
    const long long* A = acc + (long)v * STRIDE;
    const double cd = (double)c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = ((double)A[a] + 0.5 * cd) / (65536.0 * cd);   // both sums and both products are exact
        xyz[3 * o + a] = (float)(g.lo[a] + ((double)i[a] + q) * g.v);  // three roundings, no fma (see the top of the file)
    }
    if (NRM) {
        const double x = (double)A[3], y = (double)A[4], z = (double)A[5];
        const double len = sqrt((x * x + y * y) + z * z);
        const bool zero = A[3] == 0 && A[4] == 0 && A[5] == 0;
        normal[3 * o] = zero ? 0.0f : (float)(x / len);
        normal[3 * o + 1] = zero ? 0.0f : (float)(y / len);
        normal[3 * o + 2] = zero ? 0.0f : (float)(z / len);
    }
    if (COL) {
        const long long* C = A + (NRM ? 6 : 3);
#pragma unroll
        for (int a = 0; a < 3; ++a) color[3 * o + a] = (unsigned char)((2 * C[a] + c) / (2 * (long long)c));
    }
    out_count[o] = c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
struct CloudScratch {
    size_t scan, before, total, bytes;
};

// n: the points (heads) or the voxels (neighbours)
static CloudScratch cloud_layout(long long n) {
    ScratchLayout L;
    CloudScratch s = {};
    s.scan = L.take(geom_scan_bytes(n));
    s.before = L.take((size_t)(n > 0 ? n : 1) * 4);
    s.total = L.take(8);
    s.bytes = L.bytes;
    return s;
}

static int cloud_axis(double lo, double hi, double v, int* n) {
    const double c = std::ceil((hi - lo) / v);
    if (!(c >= 1.0 && c <= (double)CLOUD_AXIS_MAX)) return 0;
    *n = (int)c;
    return 1;
}

static int cloud_grid(double x_min, double x_max, double y_min, double y_max, double z_min, double z_max, double voxel, CloudGrid* g) {
    const double b[6] = {x_min, x_max, y_min, y_max, z_min, z_max};
    for (int a = 0; a < 6; ++a) D3D_REQUIRE(std::isfinite(b[a]), "border value %d is %g: all six must be finite", a, b[a]);
    D3D_REQUIRE(x_min < x_max && y_min < y_max && z_min < z_max, "border [%g, %g, %g, %g, %g, %g]: every min must be below its max",
                x_min, x_max, y_min, y_max, z_min, z_max);
    D3D_REQUIRE(std::isfinite(voxel) && voxel > 0.0, "voxel %g must be finite and > 0", voxel);
    g->v = voxel;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = b[2 * a];
        D3D_REQUIRE(cloud_axis(b[2 * a], b[2 * a + 1], voxel, &g->n[a]), "grid: axis %d has ceil(%g / %g) voxels (1 .. 2^21 - 1)", a,
                    b[2 * a + 1] - b[2 * a], voxel);
    }
    return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_cloud_scratch_bytes(long long n) {
    if (!count_ok(n)) return 0;
    return cloud_layout(n).bytes;
}

extern "C" int d3d_cloud_keys(const float* xyz, long long n_points, double x_min, double x_max, double y_min, double y_max, double z_min,
                              double z_max, double voxel, long long* keys, long long* frac, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_points), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE((xyz && keys && frac) || n_points == 0, "null pointer (xyz, keys, frac) with %lld points", n_points);
    CloudGrid g;
    const int rc = cloud_grid(x_min, x_max, y_min, y_max, z_min, z_max, voxel, &g);
    if (rc != D3D_OK) return rc;
    const size_t n = (size_t)n_points;
    const SearchRange R[3] = {{xyz, n * 12}, {keys, n * 8}, {frac, n * 8}};
    D3D_REQUIRE(search_apart(R, 3), "xyz, keys and frac must not alias");
    if (n_points == 0) return D3D_OK;
    hipLaunchKernelGGL(cloud_keys_kernel, dim3(ceil_div(n_points, CL_BLOCK)), dim3(CL_BLOCK), 0, (hipStream_t)stream, xyz, (long)n_points, g,
                       keys, frac);
    D3D_LAUNCH_CHECK("cloud_keys_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_cloud_heads(const long long* sorted_keys, long long n_points, void* scratch, size_t scratch_bytes, int* vox,
                               long long* n_voxels, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_points), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE(scratch && n_voxels, "null pointer (scratch, n_voxels)");
    D3D_REQUIRE((sorted_keys && vox) || n_points == 0, "null pointer (sorted_keys, vox) with %lld points", n_points);
    const CloudScratch L = cloud_layout(n_points);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed (d3d_cloud_scratch_bytes)", scratch_bytes, L.bytes);
    const size_t n = (size_t)n_points;
    const SearchRange R[4] = {{sorted_keys, n * 8}, {vox, n * 4}, {scratch, scratch_bytes}, {n_voxels, 8}};
    D3D_REQUIRE(search_apart(R, 4), "sorted_keys, vox, scratch and n_voxels must not alias");
    hipStream_t st = (hipStream_t)stream;
    if (n_points > 0) {
        hipLaunchKernelGGL(cloud_heads_kernel, dim3(ceil_div(n_points, CL_BLOCK)), dim3(CL_BLOCK), 0, st, sorted_keys, (long)n_points, vox);
        D3D_LAUNCH_CHECK("cloud_heads_kernel launch");
    }
    return geom_scan(vox, vox, n_points, (char*)scratch + L.scan, n_voxels, st);
}

extern "C" int d3d_cloud_accumulate(const long long* sorted_keys, const long long* order, const int* vox, const long long* frac,
                                    const float* normal, const int* color, long long n_points, long long n_voxels, long long* ukeys,
                                    int* count, long long* acc, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_points), "n_points=%lld (0 .. 2^31 - 1)", n_points);
    D3D_REQUIRE(n_voxels >= 0 && n_voxels <= n_points, "n_voxels=%lld (0 .. n_points = %lld)", n_voxels, n_points);
    D3D_REQUIRE((sorted_keys && order && vox && frac) || n_points == 0, "null pointer (sorted_keys, order, vox, frac) with %lld points",
                n_points);
    D3D_REQUIRE((ukeys && count && acc) || n_voxels == 0, "null pointer (ukeys, count, acc) with %lld voxels", n_voxels);
    const size_t n = (size_t)n_points, m = (size_t)n_voxels;
    const size_t stride = 3 + (normal ? 3 : 0) + (color ? 3 : 0);
    const SearchRange R[9] = {{sorted_keys, n * 8}, {order, n * 8}, {vox, n * 4},  {frac, n * 8},         {normal, n * 12},
                             {color, n * 12},      {ukeys, m * 8}, {count, m * 4}, {acc, m * stride * 8}};
    D3D_REQUIRE(search_apart(R, 9), "the inputs, ukeys, count and acc must not alias");
    if (n_voxels == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = hip_status(hipMemsetAsync(count, 0, m * 4, st), "cloud: clear count");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(acc, 0, m * stride * 8, st), "cloud: clear acc");
    if (rc != D3D_OK) return rc;
    const dim3 grid(ceil_div(n_points, CL_BLOCK)), block(CL_BLOCK);
#define CL_ACCUMULATE(NRM, COL)                                                                                                       \
    hipLaunchKernelGGL((cloud_accumulate_kernel<NRM, COL>), grid, block, 0, st, sorted_keys, order, vox, frac, normal, color, (long)n_points, \
                       (int)n_voxels, ukeys, count, acc)
    if (normal && color) CL_ACCUMULATE(true, true);
    else if (normal) CL_ACCUMULATE(true, false);
    else if (color) CL_ACCUMULATE(false, true);
    else CL_ACCUMULATE(false, false);
#undef CL_ACCUMULATE
    D3D_LAUNCH_CHECK("cloud_accumulate_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_cloud_neighbours(const long long* ukeys, const int* count, long long n_voxels, int nx, int ny, int nz, int min_points,
                                    void* scratch, size_t scratch_bytes, int* keep, int* pos, long long* n_kept, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_voxels), "n_voxels=%lld (0 .. 2^31 - 1)", n_voxels);
    D3D_REQUIRE(scratch && n_kept, "null pointer (scratch, n_kept)");
    D3D_REQUIRE((ukeys && count && keep && pos) || n_voxels == 0, "null pointer (ukeys, count, keep, pos) with %lld voxels", n_voxels);
    if (search_grid_ok(nx, ny, nz, "voxels") != D3D_OK) return D3D_ERR_INVALID_ARG;
    D3D_REQUIRE(min_points >= 1, "min_points=%d (>= 1)", min_points);
    const CloudScratch L = cloud_layout(n_voxels);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed (d3d_cloud_scratch_bytes)", scratch_bytes, L.bytes);
    const size_t m = (size_t)n_voxels;
    const SearchRange R[6] = {{ukeys, m * 8}, {count, m * 4}, {keep, m * 4}, {pos, m * 4}, {scratch, scratch_bytes}, {n_kept, 8}};
    D3D_REQUIRE(search_apart(R, 6), "ukeys, count, keep, pos, scratch and n_kept must not alias");
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)scratch;
    int* before = (int*)(s + L.before);
    int rc = geom_scan(count, before, n_voxels, s + L.scan, (long long*)(s + L.total), st);   // the total is n_points at most: it fits
    if (rc != D3D_OK) return rc;
    if (n_voxels > 0) {
        hipLaunchKernelGGL(cloud_neighbours_kernel, dim3(ceil_div(n_voxels, CL_BLOCK)), dim3(CL_BLOCK), 0, st, ukeys, count, before,
                           (int)n_voxels, nx, ny, nz, min_points, keep);
        D3D_LAUNCH_CHECK("cloud_neighbours_kernel launch");
    }
    return geom_scan(keep, pos, n_voxels, s + L.scan, n_kept, st);
}

extern "C" int d3d_cloud_finalize(const long long* ukeys, const int* count, const long long* acc, const int* keep, const int* pos,
                                  long long n_voxels, long long n_kept, double x_min, double x_max, double y_min, double y_max,
                                  double z_min, double z_max, double voxel, float* xyz, float* normal, unsigned char* color,
                                  int* out_count, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_voxels), "n_voxels=%lld (0 .. 2^31 - 1)", n_voxels);
    D3D_REQUIRE(n_kept >= 0 && n_kept <= n_voxels, "n_kept=%lld (0 .. n_voxels = %lld)", n_kept, n_voxels);
    D3D_REQUIRE((ukeys && count && acc && keep && pos) || n_voxels == 0, "null pointer (ukeys, count, acc, keep, pos) with %lld voxels",
                n_voxels);
    D3D_REQUIRE((xyz && out_count) || n_kept == 0, "null pointer (xyz, out_count) with %lld kept voxels", n_kept);
    CloudGrid g;
    const int rc = cloud_grid(x_min, x_max, y_min, y_max, z_min, z_max, voxel, &g);
    if (rc != D3D_OK) return rc;
    const size_t m = (size_t)n_voxels, k = (size_t)n_kept;
    const size_t stride = 3 + (normal ? 3 : 0) + (color ? 3 : 0);
    const SearchRange R[9] = {{ukeys, m * 8}, {count, m * 4},   {acc, m * stride * 8}, {keep, m * 4},     {pos, m * 4},
                             {xyz, k * 12},  {normal, k * 12}, {color, k * 3},        {out_count, k * 4}};
    D3D_REQUIRE(search_apart(R, 9), "the inputs, xyz, normal, color and out_count must not alias");
    if (n_kept == 0) return D3D_OK;
    const dim3 grid(ceil_div(n_voxels, CL_BLOCK)), block(CL_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define CL_FINALIZE(NRM, COL)                                                                                                   \
    hipLaunchKernelGGL((cloud_finalize_kernel<NRM, COL>), grid, block, 0, st, ukeys, count, acc, keep, pos, (int)n_voxels, (int)n_kept, g, \
                       xyz, normal, color, out_count)
    if (normal && color) CL_FINALIZE(true, true);
    else if (normal) CL_FINALIZE(true, false);
    else if (color) CL_FINALIZE(false, true);
    else CL_FINALIZE(false, false);
#undef CL_FINALIZE
    D3D_LAUNCH_CHECK("cloud_finalize_kernel launch");
    return D3D_OK;
}
