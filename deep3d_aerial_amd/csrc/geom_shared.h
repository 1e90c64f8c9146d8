// The primitives the geometry stages share (fusion, normals, dsm, dtm, objects, outlines, ortho, ortho_mesh, view_select, cloud and
// its outliers, normals, compare and register stages, mesh, mesh_sample, mesh_clean, mesh_decimate, mesh_holes, mesh_refine,
// mesh_subdivide, mesh_collapse, mesh_flip, texture and its smooth, level, local and outliers passes); not part of the public ABI.
// The kernels behind the host functions declared here are in geom.hip.
#pragma once
#include <cstdint>

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

// ---------------------------------------------------------------------------------------------------------------------------
// wave and workgroup
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float geom_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float geom_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int geom_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int geom_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ unsigned geom_min(unsigned a, unsigned b) { return min(a, b); }
__device__ __forceinline__ unsigned geom_max(unsigned a, unsigned b) { return max(a, b); }

// The minimum / maximum / sum of x over the 64 lanes of the wave, in every lane.
template <typename T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = geom_min(x, __shfl_xor(x, o, 64));
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = geom_max(x, __shfl_xor(x, o, 64));
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// The counters of a wave: the sum of each c (int, or bool as 0 / 1) over the wave, the i-th one added to counts[i] by lane 0 when
// it is not zero, with one integer atomicAdd whose result is unused.  Every lane of the wave calls it.
template <typename... T>
__device__ __forceinline__ void wave_counts_add(int* counts, T... c) {
    const int sums[] = {wave_sum((int)c)...};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < (int)sizeof...(T); ++i)
            if (sums[i]) atomicAdd(counts + i, sums[i]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// runs of a wave: a run is a maximal set of consecutive lanes with equal v.  A kernel whose lanes hold few runs (sorted keys, the
// samples of a face, the cells of a row) reduces each run into its last lane and sends one set of atomics per run instead of one
// per lane; every reduction here is on integers, so the grouping does not change a bit.
//   - Every lane of the wave calls these (they shuffle and ballot): no lane may have returned before.
//   - v need not be sorted: equal values that are not adjacent are separate runs.
//   - Lanes with v < 0 ("nothing here") form runs like any other; the caller discards them.
//   - A run ends at the wave's edge: one that crosses waves is sent once per wave.
// ---------------------------------------------------------------------------------------------------------------------------
// The lowest lane of this lane's run: the highest run head (lane 0, or a lane whose v differs from the lane before) at or below it.
__device__ __forceinline__ int wave_run_first(int v, int lane) {
    const int before = __shfl_up(v, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != v);
    return 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));
}

// True in the highest lane of each run.
__device__ __forceinline__ bool wave_run_last(int v, int lane) {
    const int next = __shfl_down(v, 1, 64);
    return lane == 63 || next != v;
}

// The sum / maximum of x over the lanes first .. lane, first = wave_run_first(v, lane).
template <typename T>
__device__ __forceinline__ T wave_run_sum(T x, int first, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane - o >= first) x += y;
    }
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_run_max(T x, int first, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane - o >= first) x = geom_max(x, y);
    }
    return x;
}

// Exclusive scan of one value per lane over the workgroup (blockDim.x a multiple of 64); *total gets the sum.
template <typename T>
__device__ __forceinline__ T block_exclusive(T x, T* lds, T* total) {
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

// ---------------------------------------------------------------------------------------------------------------------------
// device scan
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int GEOM_SCAN_TILE = 256 * 16;   // values per workgroup of the scan: 256 lanes of 16

inline long long geom_scan_tiles(long long n) { return (n + GEOM_SCAN_TILE - 1) / GEOM_SCAN_TILE; }

// Exclusive scan of n int32 values into out (out may be in), *total (device int64, or null) their sum; tile_sums: one S per
// tile of GEOM_SCAN_TILE values.  S is int64 where the caller checks that the total fits in int32, int32 where it is known to
// (the DSM's scratch has 4 bytes per tile, and its total is at most n_points < 2^31).
template <typename S>
int geom_scan_sums(const int* in, int* out, long long n, S* tile_sums, long long* total, hipStream_t st);

// d3d_mesh_scan_scratch_bytes(n) for n >= 0: the int64 tile sums
inline size_t geom_scan_bytes(long long n) { return (size_t)(geom_scan_tiles(n) > 0 ? geom_scan_tiles(n) : 1) * 8; }

// The scan with a scratch of geom_scan_bytes(n) bytes.
inline int geom_scan(const int* in, int* out, long long n, void* scratch, long long* total, hipStream_t st) {
    return geom_scan_sums(in, out, n, (long long*)scratch, total, st);
}

// ---------------------------------------------------------------------------------------------------------------------------
// scratch layout: `at = L.take(bytes)` hands out consecutive 256-byte aligned offsets, L.bytes is the size so far
// ---------------------------------------------------------------------------------------------------------------------------
// A count of points, voxels, faces or samples an entry point takes: 0 .. 2^31 - 1, so that an index fits in int32.
inline bool count_ok(long long n) { return n >= 0 && n < (1ll << 31); }

// A W x H raster an entry point takes: both sides >= 1 and at most max_cells cells.
inline bool raster_ok(int W, int H, long long max_cells) { return W >= 1 && H >= 1 && (long long)W * H <= max_cells; }

// The na bytes at a and the nb bytes at b do not overlap.
inline bool geom_apart(const void* a, size_t na, const void* b, size_t nb) {
    return (uintptr_t)a + na <= (uintptr_t)b || (uintptr_t)b + nb <= (uintptr_t)a;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct ScratchLayout {
    size_t bytes = 0;
    size_t take(size_t b) {
        const size_t at = bytes;
        bytes += align256(b);
        return at;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// union-find by hooking and pointer jumping
// ---------------------------------------------------------------------------------------------------------------------------
// parent[i] = i
int geom_iota(int* parent, long long n, hipStream_t st);
// parent[i] = the root of i
int geom_jump(int* parent, long long n, hipStream_t st);

// Joins the sets of two elements whose parents the caller has loaded as pa and pb: the larger parent gets the smaller one
// (atomicMin), so parents only decrease and stay in their set, and the fixed point of hooking and jumping in turn is the
// smallest index of each set.  The caller's plain loads may return a parent that another workgroup has already lowered, or not
// yet: either is a member of the same set no larger than the element, so a stale read only costs a round.  A launch that sets
// no flag has made no atomic, so its loads saw the previous launch's values, and they agree on every pair.
__device__ __forceinline__ void geom_hook(int* parent, int pa, int pb, int* changed) {
    if (pa != pb) {
        atomicMin(parent + max(pa, pb), min(pa, pb));
        *changed = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// faces
// ---------------------------------------------------------------------------------------------------------------------------
// The indices of face f; false when one is out of range or, with DISTINCT, two are equal (the Python side refuses such faces;
// the kernels skip them).
template <bool DISTINCT>
__device__ __forceinline__ bool geom_face(const int* __restrict__ faces, long f, long long n, int* a, int* b, int* c) {
    *a = faces[3 * f];
    *b = faces[3 * f + 1];
    *c = faces[3 * f + 2];
    const bool ok = *a >= 0 && *a < n && *b >= 0 && *b < n && *c >= 0 && *c < n;
    return DISTINCT ? ok && *a != *b && *b != *c && *c != *a : ok;
}

// Vertex i of an fp32 [n, 3] array as three doubles; the caller has checked 0 <= i < n.
__device__ __forceinline__ void geom_load3(const float* __restrict__ v, long i, double* p) {
    p[0] = (double)v[3 * i];
    p[1] = (double)v[3 * i + 1];
    p[2] = (double)v[3 * i + 2];
}

// ---------------------------------------------------------------------------------------------------------------------------
// the validity tests of an edge collapse (mesh_decimate, mesh_collapse)
// ---------------------------------------------------------------------------------------------------------------------------
// nrm = (p1 - p0) x (p2 - p0)
__device__ __forceinline__ void dq_normal(const double* p0, const double* p1, const double* p2, double* nrm) {
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    nrm[0] = uy * vz - uz * vy;
    nrm[1] = uz * vx - ux * vz;
    nrm[2] = ux * vy - uy * vx;
}

// The vertices the sorted neighbour rows offset[a] .. offset[a + 1] and offset[b] .. offset[b + 1] share, by a merge.
__device__ __forceinline__ int dq_shared(const long long* __restrict__ offset, const int* __restrict__ nbr, int a, int b) {
    const long long a1 = offset[a + 1], b1 = offset[b + 1];
    int shared = 0;
    for (long long i = offset[a], j = offset[b]; i < a1 && j < b1;) {
        const int u = nbr[i], w = nbr[j];
        shared += u == w ? 1 : 0;
        i += u <= w ? 1 : 0;
        j += w <= u ? 1 : 0;
    }
    return shared;
}

// The faces of row v that do not hold `other`, with v (and other) at position t: true when one of them turns over or collapses.
__device__ __forceinline__ bool dq_flips(const float* __restrict__ vertices, const int* __restrict__ faces, const int* __restrict__ foff,
                                         const int* __restrict__ finc, int v, int other, const double* t) {
    const int o1 = foff[v + 1];
    for (int o = foff[v]; o < o1; ++o) {
        const long f = finc[o];
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (i0 == other || i1 == other || i2 == other) continue;
        double p0[3], p1[3], p2[3], n0[3], n1[3];
        geom_load3(vertices, i0, p0);
        geom_load3(vertices, i1, p1);
        geom_load3(vertices, i2, p2);
        dq_normal(p0, p1, p2, n0);
        double* moved = i0 == v ? p0 : (i1 == v ? p1 : p2);
        moved[0] = t[0], moved[1] = t[1], moved[2] = t[2];
        dq_normal(p0, p1, p2, n1);
        const double dot = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2];
        if (!(dot > 0.0)) return true;
    }
    return false;
}

// n_vertices and n_faces in the range the collapse passes index with int32: 0 .. 2^31 - 1 vertices, 6 n_faces < 2^31.
inline bool dq_sizes_ok(long long n, long long m) { return n >= 0 && n < (1ll << 31) && m >= 0 && 6 * m < (1ll << 31); }

// The distinct edges of face (a, b, c): the pairs (a,b) (b,c) (c,a) with unequal ends, each unordered pair once.
__device__ __forceinline__ int geom_face_edges(int a, int b, int c, int* x, int* y) {
    if (a == b && b == c) return 0;
    if (a == b || c == a) {   // (a, a, c) or (a, b, a): one edge
        x[0] = a;
        y[0] = a == b ? c : b;
        return 1;
    }
    if (b == c) {
        x[0] = a;
        y[0] = b;
        return 1;
    }
    x[0] = a, y[0] = b;
    x[1] = b, y[1] = c;
    x[2] = c, y[2] = a;
    return 3;
}

// Compaction of the faces with keep[f] != 0, in input order: pos = the exclusive scan of keep, *n_kept its total, the kept
// faces' indices (through remap when it is not null) to out_faces, and referenced[v] = 1 for each of them.
struct KeepScratch {
    size_t keep, pos, scan, bytes;
};

inline KeepScratch geom_keep_layout(long long m) {
    const size_t nf = (size_t)(m > 0 ? m : 1);
    ScratchLayout L;
    KeepScratch s;
    s.keep = L.take(nf * 4);
    s.pos = L.take(nf * 4);
    s.scan = L.take(geom_scan_bytes(m));
    s.bytes = L.bytes;
    return s;
}

int geom_scatter_kept(const int* faces, long long m, const int* remap, void* scratch, const KeepScratch& L, int* out_faces,
                      int* referenced, long long* n_kept, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------------------
// fp64 pinhole projection of a d3d_mesh_view_t or d3d_ortho_view_t: p = R X + t, q = K p, each row summed left to right,
// u = q0 / q2, v = q1 / q2 (built with -ffp-contract=off: no contraction)
// ---------------------------------------------------------------------------------------------------------------------------
struct GeomPq {
    double p2, q0, q1, q2;
};

template <typename View>
__device__ __forceinline__ GeomPq geom_project(const View& V, double X0, double X1, double X2) {
    const double p0 = V.R[0] * X0 + V.R[1] * X1 + V.R[2] * X2 + V.t[0];
    const double p1 = V.R[3] * X0 + V.R[4] * X1 + V.R[5] * X2 + V.t[1];
    const double p2 = V.R[6] * X0 + V.R[7] * X1 + V.R[8] * X2 + V.t[2];
    GeomPq r;
    r.p2 = p2;
    r.q0 = V.K[0] * p0 + V.K[1] * p1 + V.K[2] * p2;
    r.q1 = V.K[3] * p0 + V.K[4] * p1 + V.K[5] * p2;
    r.q2 = V.K[6] * p0 + V.K[7] * p1 + V.K[8] * p2;
    return r;
}

// (u, v) of X in view V when it lies in front of the view (p2 > 0, q2 > 0) and inside its image (0 <= u <= W - 1,
// 0 <= v <= H - 1, both ends included), else false; *p2 is the depth along the view's axis.  A NaN fails every test.
template <typename View>
__device__ __forceinline__ bool geom_uv(const View& V, double X0, double X1, double X2, double* u, double* v, double* p2) {
    const GeomPq r = geom_project(V, X0, X1, X2);
    if (!(r.p2 > 0.0 && r.q2 > 0.0)) return false;
    *u = r.q0 / r.q2;
    *v = r.q1 / r.q2;
    *p2 = r.p2;
    return *u >= 0.0 && *u <= (double)(V.W - 1) && *v >= 0.0 && *v <= (double)(V.H - 1);
}

// The depth map of V at the pixel nearest to (u, v): (floor(v + 0.5), floor(u + 0.5)).  The caller has placed (u, v) inside the
// image (geom_uv) and checked V.depth, so the clamp only guards the load.  The test on the value (finite, > 0, p2 <= D tol1,
// with or without a slack) stays with the caller: as a predicate here it moved the callers' machine code.
template <typename View>
__device__ __forceinline__ float geom_depth_at(const View& V, double u, double v) {
    const int px = min(max((int)floor(u + 0.5), 0), V.W - 1), py = min(max((int)floor(v + 0.5), 0), V.H - 1);
    return V.depth[(long)py * V.W + px];
}

// ---------------------------------------------------------------------------------------------------------------------------
// the colour of an RGBA8 image at (u, v)
// ---------------------------------------------------------------------------------------------------------------------------
// The bilinear blend of four RGBA8 taps, per channel (R, G, B = bits 0, 8, 16) in fp64 and not rounded: the weights
// w00 = (1 - fx)(1 - fy), w10 = fx (1 - fy), w01 = (1 - fx) fy, w11 = fx fy, the sum ((w00 t00 + w10 t10) + w01 t01) + w11 t11.
__device__ __forceinline__ void geom_blend(unsigned t00, unsigned t10, unsigned t01, unsigned t11, double fx, double fy, double (&t)[3]) {
    const double w00 = (1.0 - fx) * (1.0 - fy), w10 = fx * (1.0 - fy), w01 = (1.0 - fx) * fy, w11 = fx * fy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
        t[ch] = w00 * (double)((t00 >> sh) & 255u) + w10 * (double)((t10 >> sh) & 255u) + w01 * (double)((t01 >> sh) & 255u) +
                w11 * (double)((t11 >> sh) & 255u);
    }
}

// The bilinear tap of a W x H RGBA8 image at (u, v) (ortho.py "Colour"): x0 = floor(u) clamped to 0 .. W - 1, fx = u - floor(u)
// (of the unclamped floor), x1 = min(x0 + 1, W - 1), the same in y, then geom_blend.  rgba is not null, W, H >= 1.
__device__ __forceinline__ void geom_tap(const unsigned* __restrict__ rgba, int W, int H, double u, double v, double (&t)[3]) {
    const double fu = floor(u), fv = floor(v);
    const double fx = u - fu, fy = v - fv;
    const int x0 = (int)fmin(fmax(fu, 0.0), (double)(W - 1)), y0 = (int)fmin(fmax(fv, 0.0), (double)(H - 1));
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const unsigned t00 = rgba[(long)y0 * W + x0], t10 = rgba[(long)y0 * W + x1];
    const unsigned t01 = rgba[(long)y1 * W + x0], t11 = rgba[(long)y1 * W + x1];
    geom_blend(t00, t10, t01, t11, fx, fy, t);
}

// ---------------------------------------------------------------------------------------------------------------------------
// view keys and sorted key lists
// ---------------------------------------------------------------------------------------------------------------------------
// key = (bits(fp32(s)) << 32) | id for a score s >= 0 (the caller has checked that it is finite): keys order as (s, id), the
// smallest wins.  geom_key_id is the id again.
__device__ __forceinline__ long long geom_view_key(double s, int id) {
    return ((long long)__float_as_uint((float)s) << 32) | (long long)(unsigned)id;
}

__device__ __forceinline__ int geom_key_id(long long key) { return (int)(unsigned)key; }

// Inserts k into the sorted list c (increasing, padded with `empty`, the largest key) and drops the largest; a key the list
// already holds is dropped instead.  Every index is a compile-time constant after unrolling.
template <int N>
__device__ __forceinline__ void geom_list_insert(long long (&c)[N], long long k, long long empty) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        k = k == c[i] ? empty : k;
        const long long lo = k < c[i] ? k : c[i];
        k = k < c[i] ? c[i] : k;
        c[i] = lo;
    }
}

}  // namespace d3d
