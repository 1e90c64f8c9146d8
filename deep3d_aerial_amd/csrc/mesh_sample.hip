// Deterministic samples of a surface mesh at a stated spacing, and a comparison's error brought back onto the faces (DESIGN.md
// §4.30; deep3d_aerial_amd/mesh_compare.py states the rule, include/deep3d_planesweep.h too, tests/mesh_compare_scene.py restates it
// in numpy).  The rule is this project's own; it does not claim to match any tool.
//
// Inputs: vertices [nv,3] fp32, faces [m,3] int32, a spacing s, finite and > 0.
// Per face f with corners (A, B, C) in the face's own order, all arithmetic fp64, every operation rounded once
// (-ffp-contract=off):
//   L2  = the largest of the three squared edge lengths, each (dx dx + dy dy) + dz dz
//   n_f = 0 when a corner coordinate is not finite or L2 is not a finite number > 0 (or an index is outside 0 .. nv - 1, which
//         the Python side refuses)
//   else q = sqrt(L2) / s, n_f = 1 for q <= 1, else ceil(q); an n_f above N_MAX = 32768 is N_MAX and the face counts as clipped
//   the face gets n_f^2 samples: the centroids of the n_f^2 congruent sub-triangles of its n_f-fold edge subdivision
// Sample t (0 .. n^2 - 1) of a face with n = n_f:
//   row r = floor(sqrt(t)) (an exact integer square root), c = t - r^2 in 0 .. 2r, k = c >> 1
//   integer weights (p, q, w) with p + q + w = 3n:
//     c even (upright):   p = 3(n - r) - 2, q = 3k + 1, w = 3(r - k) + 1
//     c odd  (inverted):  p = 3(n - r) - 1, q = 3k + 2, w = 3(r - k) - 1
//   per axis x = ((p A_x + q B_x) + w C_x) / (3n) in fp64, then rounded to fp32
// Order: (face in input order, t).  Outputs: offsets [m+1] the exclusive scan of n_f^2, xyz [S,3] fp32, face [S] int32.
//
// count:      one lane per face (geom_face, geom_load3), n_f^2 as int32; the clipped faces and the samples are summed per
//             workgroup (shuffles, then LDS) and added with one integer atomicAdd per workgroup each.  The samples are summed here
//             in int64 and not taken from the scan's tile sums: those are int32 per tile, and two faces of 2^30 samples in one tile
//             wrap them.  geom_scan then gives offsets, valid only when the total is below 2^31 (the d3d_mesh_count convention).
// emit:       one lane per SAMPLE, a tile of 256 consecutive sample indices at a time, eight consecutive tiles a workgroup.  Two
//             lanes find the face of the tile's first and last index (the last offset <= g, among all m + 1 offsets) and share them through LDS; every lane then searches only
//             between those two faces: no step when the tile lies inside one face, at most 8 when every face has one sample.  A
//             face without samples has the offset of the next face, so the last offset <= g is never one of them, however many
//             lie between two sampled faces (a tile may span more than 256 faces because of them).  n is the integer square root
//             of the face's count, r that of t: (long long)sqrt((double)t) and an integer fix-up in both directions.  12 + 4 bytes
//             stored a lane, consecutive over the lanes.
// face error: one lane per sample of a comparison: e [S] and face [S] in, per face sum int64 and keyed int32 over the samples
//             with e >= 0, worst int32 their maximum (-1 for a face without one).  The samples of a face are consecutive, so each
//             run of equal faces within a wave is reduced by shuffles (the run reduction of geom_shared.h: the sums and
//             maxima are integers, so any grouping gives the same bits) and its last lane issues the atomics; a run that crosses
//             waves adds once per wave.  The runs are found from the neighbouring lanes, so an unsorted face array gives the same
//             result too.  Built with -DD3D_MESH_SAMPLE_PLAIN every keyed sample issues its own atomics (the form
//             tools/mesh_compare_bench.py times beside this one).
// Atomics: integer atomicAdd and atomicMax, results unused: the same bits for any order of the lanes.
#include <climits>
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int MS_BLOCK = 256;
constexpr int MS_WAVES = MS_BLOCK / 64;
constexpr int MS_N_MAX = 32768;   // the largest n_f: n_f^2 = 2^30 fits in int32
constexpr int MS_EMIT_TILES = 8;   // tiles of 256 samples a workgroup of emit takes, one after the other (1 was slower: DESIGN.md §4.30)

// The sum of x over the workgroup, in every lane; lds: one T per wave.
template <typename T>
__device__ __forceinline__ T ms_block_sum(T x, T* lds) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    T all = 0;
#pragma unroll
    for (int w = 0; w < MS_WAVES; ++w) all += lds[w];
    return all;
}

__device__ __forceinline__ double ms_edge2(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ bool ms_finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// totals: [0] the samples, [1] the clipped faces (zeroed by the host before the launch)
__global__ __launch_bounds__(MS_BLOCK) void mesh_sample_count_kernel(const float* __restrict__ vertices, long long nv,
                                                                     const int* __restrict__ faces, long m, double spacing,
                                                                     int* __restrict__ counts, unsigned long long* __restrict__ totals) {
    __shared__ long long sum_lds[MS_WAVES];
    __shared__ int clip_lds[MS_WAVES];
    const long f = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    int n = 0, clipped = 0;
    int a, b, c;
    if (f < m && geom_face<false>(faces, f, nv, &a, &b, &c)) {
        double A[3], B[3], C[3];
        geom_load3(vertices, a, A);
        geom_load3(vertices, b, B);
        geom_load3(vertices, c, C);
        const double ab = ms_edge2(A, B), bc = ms_edge2(B, C), ca = ms_edge2(C, A);
        const double ab_bc = ab > bc ? ab : bc;   // (a NaN comes only from a corner that is not finite, tested below)
        const double L2 = ab_bc > ca ? ab_bc : ca;
        if (ms_finite3(A) && ms_finite3(B) && ms_finite3(C) && isfinite(L2) && L2 > 0.0) {
            const double q = sqrt(L2) / spacing;
            if (q <= 1.0) {
                n = 1;
            } else if (q > (double)MS_N_MAX) {   // an infinite q too (a tiny spacing)
                n = MS_N_MAX;
                clipped = 1;
            } else {
                n = (int)ceil(q);
            }
        }
    }
    if (f < m) counts[f] = n * n;
    const long long samples = ms_block_sum((long long)n * n, sum_lds);
    const int n_clipped = ms_block_sum(clipped, clip_lds);
    if (threadIdx.x == 0) {
        if (samples != 0) atomicAdd(totals, (unsigned long long)samples);
        if (n_clipped != 0) atomicAdd(totals + 1, (unsigned long long)n_clipped);
    }
}

// The last index i in [lo, hi] with offsets[i] <= g; the caller knows offsets[lo] <= g.
__device__ __forceinline__ int ms_last_le(const int* __restrict__ offsets, int lo, int hi, int g) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (offsets[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// floor(sqrt(t)) for 0 <= t <= 2^30
__device__ __forceinline__ int ms_isqrt(int t) {
    long long r = (long long)sqrt((double)t);
    while (r * r > (long long)t) --r;
    while ((r + 1) * (r + 1) <= (long long)t) ++r;
    return (int)r;
}

// Sample g of the mesh, whose face lies in lo .. hi.
__device__ __forceinline__ void ms_emit_sample(const float* __restrict__ vertices, long long nv, const int* __restrict__ faces,
                                               const int* __restrict__ offsets, int lo, int hi, int g, float* __restrict__ xyz,
                                               int* __restrict__ face) {
    const int f = ms_last_le(offsets, lo, hi, g);   // in 0 .. m - 1 whatever the offsets hold
    const float bad = __int_as_float(0x7fc00000);
    float x[3] = {bad, bad, bad};
    const int t = g - offsets[f], count = offsets[f + 1] - offsets[f];
    int a, b, c;
    // (false only for offsets that d3d_mesh_sample_count did not write for this mesh: a guard on the loads)
    if (t >= 0 && t < count && geom_face<false>(faces, f, nv, &a, &b, &c)) {
        const int n = ms_isqrt(count);
        const int r = ms_isqrt(t);
        const int col = t - r * r, k = col >> 1;
        const int odd = col & 1;
        const double p = (double)(3 * (n - r) - 2 + odd), q = (double)(3 * k + 1 + odd), w = (double)(3 * (r - k) + 1 - 2 * odd);
        const double d = (double)(3 * n);
        double A[3], B[3], C[3];
        geom_load3(vertices, a, A);
        geom_load3(vertices, b, B);
        geom_load3(vertices, c, C);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) x[ax] = (float)(((p * A[ax] + q * B[ax]) + w * C[ax]) / d);
    }
    xyz[3 * (long)g] = x[0];
    xyz[3 * (long)g + 1] = x[1];
    xyz[3 * (long)g + 2] = x[2];
    face[g] = f;
}

// A workgroup takes MS_EMIT_TILES consecutive tiles of 256 samples, one after the other.
__global__ __launch_bounds__(MS_BLOCK) void mesh_sample_emit_kernel(const float* __restrict__ vertices, long long nv,
                                                                    const int* __restrict__ faces, int m, const int* __restrict__ offsets,
                                                                    int n_samples, float* __restrict__ xyz, int* __restrict__ face) {
    __shared__ int edge[2];
    for (int tile = 0; tile < MS_EMIT_TILES; ++tile) {
        const long first = ((long)blockIdx.x * MS_EMIT_TILES + tile) * MS_BLOCK;
        if (first >= n_samples) break;   // the same for every lane of the workgroup
        const int g0 = (int)first;
        const int g1 = (int)min(first + MS_BLOCK - 1, (long)n_samples - 1);   // the tile's last sample
        if (threadIdx.x < 2) edge[threadIdx.x] = ms_last_le(offsets, 0, m - 1, threadIdx.x ? g1 : g0);
        __syncthreads();
        if (first + threadIdx.x < n_samples) ms_emit_sample(vertices, nv, faces, offsets, edge[0], edge[1], g0 + threadIdx.x, xyz, face);
        __syncthreads();   // before the next tile's faces replace these
    }
}

// sum and keyed zeroed and worst set to -1 by the host before the launch
__global__ __launch_bounds__(MS_BLOCK) void mesh_sample_face_error_kernel(const int* __restrict__ e, const int* __restrict__ face, long n,
                                                                          int m, unsigned long long* __restrict__ sum,
                                                                          int* __restrict__ keyed, int* __restrict__ worst) {
    const long g = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    int f = -1, c = 0, hi = -1;
    long long s = 0;
    if (g < n) {
        f = face[g];
        if (f < 0 || f >= m) f = -1;   // never true for the face array of d3d_mesh_sample_emit: a guard on the writes
        const int v = e[g];
        if (f >= 0 && v >= 0) s = v, c = 1, hi = v;
    }
#ifndef D3D_MESH_SAMPLE_PLAIN
    const int lane = threadIdx.x & 63;
    const int first = wave_run_first(f, lane);   // of this lane's run of equal faces
    s = wave_run_sum(s, first, lane);   // 64-bit: any e >= 0 sums as the plain form's atomics would
    c = wave_run_sum(c, first, lane);
    hi = wave_run_max(hi, first, lane);
    if (!wave_run_last(f, lane)) return;   // not the last lane of its run in this wave
#endif
    if (f < 0 || c == 0) return;
    atomicAdd(sum + f, (unsigned long long)s);
    atomicAdd(keyed + f, c);
    atomicMax(worst + f, hi);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------

static size_t ms_scratch(long long m) { return align256(geom_scan_bytes(m)); }

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_mesh_sample_scratch_bytes(long long n_faces) {
    if (!count_ok(n_faces)) return 0;
    return ms_scratch(n_faces);
}

extern "C" int d3d_mesh_sample_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, double spacing,
                                     void* scratch, size_t scratch_bytes, int* counts, int* offsets, long long* totals,
                                     d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_vertices), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    D3D_REQUIRE(count_ok(n_faces), "n_faces=%lld (0 .. 2^31 - 1)", n_faces);
    D3D_REQUIRE(std::isfinite(spacing) && spacing > 0.0, "spacing %g must be finite and > 0", spacing);
    D3D_REQUIRE(scratch && offsets && totals, "null pointer (scratch, offsets, totals)");
    D3D_REQUIRE((faces && counts) || n_faces == 0, "null pointer (faces, counts) with %lld faces", n_faces);
    D3D_REQUIRE(vertices || n_vertices == 0, "null pointer (vertices) with %lld vertices", n_vertices);
    const size_t need = ms_scratch(n_faces);
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_mesh_sample_scratch_bytes)", scratch_bytes, need);
    const size_t nv = (size_t)n_vertices, m = (size_t)n_faces;
    const SearchRange R[6] = {{vertices, nv * 12}, {faces, m * 12}, {scratch, scratch_bytes}, {counts, m * 4}, {offsets, (m + 1) * 4},
                              {totals, 16}};
    D3D_REQUIRE(search_apart(R, 6), "vertices, faces, scratch, counts, offsets and totals must not alias");
    hipStream_t st = (hipStream_t)stream;
    int rc = hip_status(hipMemsetAsync(totals, 0, 16, st), "mesh sample: clear totals");
    if (rc != D3D_OK) return rc;
    if (n_faces > 0) {
        hipLaunchKernelGGL(mesh_sample_count_kernel, dim3(ceil_div(n_faces, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertices, n_vertices, faces,
                           (long)n_faces, spacing, counts, (unsigned long long*)totals);
        D3D_LAUNCH_CHECK("mesh_sample_count_kernel launch");
        rc = geom_scan(counts, offsets, n_faces, scratch, nullptr, st);
        if (rc != D3D_OK) return rc;
    }
    // offsets[m] = the total (its low 32 bits: the offsets are valid only when it is below 2^31)
    return hip_status(hipMemcpyAsync(offsets + n_faces, totals, 4, hipMemcpyDeviceToDevice, st), "mesh sample: the last offset");
}

extern "C" int d3d_mesh_sample_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* offsets,
                                    long long n_samples, float* xyz, int* face, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_vertices), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    D3D_REQUIRE(count_ok(n_faces), "n_faces=%lld (0 .. 2^31 - 1)", n_faces);
    D3D_REQUIRE(count_ok(n_samples), "n_samples=%lld (0 .. 2^31 - 1)", n_samples);
    D3D_REQUIRE(n_faces > 0 || n_samples == 0, "n_samples=%lld with no face", n_samples);
    D3D_REQUIRE(offsets, "null pointer (offsets)");
    D3D_REQUIRE(faces || n_faces == 0, "null pointer (faces) with %lld faces", n_faces);
    D3D_REQUIRE(vertices || n_vertices == 0, "null pointer (vertices) with %lld vertices", n_vertices);
    D3D_REQUIRE((xyz && face) || n_samples == 0, "null pointer (xyz, face) with %lld samples", n_samples);
    const size_t nv = (size_t)n_vertices, m = (size_t)n_faces, S = (size_t)n_samples;
    const SearchRange R[5] = {{vertices, nv * 12}, {faces, m * 12}, {offsets, (m + 1) * 4}, {xyz, S * 12}, {face, S * 4}};
    D3D_REQUIRE(search_apart(R, 5), "vertices, faces, offsets, xyz and face must not alias");
    if (n_samples == 0) return D3D_OK;
    hipLaunchKernelGGL(mesh_sample_emit_kernel, dim3(ceil_div(n_samples, (long)MS_BLOCK * MS_EMIT_TILES)), dim3(MS_BLOCK), 0, (hipStream_t)stream, vertices,
                       n_vertices, faces, (int)n_faces, offsets, (int)n_samples, xyz, face);
    D3D_LAUNCH_CHECK("mesh_sample_emit_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_sample_face_error(const int* e, const int* face, long long n_samples, long long n_faces, long long* sum, int* keyed,
                                          int* worst, d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_samples), "n_samples=%lld (0 .. 2^31 - 1)", n_samples);
    D3D_REQUIRE(count_ok(n_faces), "n_faces=%lld (0 .. 2^31 - 1)", n_faces);
    D3D_REQUIRE((e && face) || n_samples == 0, "null pointer (e, face) with %lld samples", n_samples);
    D3D_REQUIRE((sum && keyed && worst) || n_faces == 0, "null pointer (sum, keyed, worst) with %lld faces", n_faces);
    const size_t S = (size_t)n_samples, m = (size_t)n_faces;
    const SearchRange R[5] = {{e, S * 4}, {face, S * 4}, {sum, m * 8}, {keyed, m * 4}, {worst, m * 4}};
    D3D_REQUIRE(search_apart(R, 5), "e, face, sum, keyed and worst must not alias");
    if (n_faces == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = hip_status(hipMemsetAsync(sum, 0, m * 8, st), "mesh face error: clear sum");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(keyed, 0, m * 4, st), "mesh face error: clear keyed");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(worst, 0xff, m * 4, st), "mesh face error: worst = -1");
    if (rc != D3D_OK) return rc;
    if (n_samples == 0) return D3D_OK;
    hipLaunchKernelGGL(mesh_sample_face_error_kernel, dim3(ceil_div(n_samples, MS_BLOCK)), dim3(MS_BLOCK), 0, st, e, face, (long)n_samples,
                       (int)n_faces, (unsigned long long*)sum, keyed, worst);
    D3D_LAUNCH_CHECK("mesh_sample_face_error_kernel launch");
    return D3D_OK;
}
