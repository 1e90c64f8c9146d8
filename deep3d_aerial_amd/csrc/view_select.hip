// View selection from a sparse model: the reference views of scene blocks and the co-visibility score of every reference view
// (deep3d_aerial_amd/view_selection.py states the rule, include/deep3d_planesweep.h too,
// tests/view_selection_scene.py restates it in numpy).
//
// The model arrives in dense indices: image k = 0 .. n_img - 1, point p = 0 .. n_pts - 1; the observations as CSR by image
// (img_offset [n_img + 1] int64, obs_point [n_obs] int32, -1 = no point), the tracks as CSR by point (trk_offset [n_pts + 1]
// int64, trk_image [n_trk] int32).
//
// blocks: one lane per point p >= p_first (the points before it have an id <= 0 and are ignored); the block table
//         [n_blocks, 4] fp64 = (x0, x1, y0, y1) in LDS.  For each block with x0 < x < x1 and y0 < y < y1 (strict, fp64, z not
//         tested) the lane stores 1 to mask[b][k] for every k of the point's track: a plain byte store of the same value from
//         whoever gets there, so no atomics.  mask [n_blocks, n_img] is cleared by the call.
// rows:   one workgroup per reference image r.  C_r [n_img] unsigned (and S_r [n_img] unsigned in angle mode) live in dynamic
//         LDS when rows * n_img <= lds_images, else in the workgroup's row of a global scratch the call clears, batch by batch
//         of at most VS_BATCH reference images; the kernel body is the same and so are the bits.  The lanes stride over the
//         observations of r; each walks the track of its point and adds 1 to C_r[s] (and W[bin] to S_r[s], s != r) with an
//         integer atomicAdd whose result is unused.  After a barrier the workgroup reduces seen_r (the s != r with C_r[s] > 0)
//         and max_r (over s != r, of C in points mode and of S in angle mode), and emits the sources -- C_r[s] > 10 and
//         10 score > max_r -- in ascending s through a scan per 256 columns into the segment seg_offset[i] .. seg_offset[i + 1]
//         of src / score / count.  A segment is sized by the host (a source has C > 10, so there are at most sum(C) / 11 of
//         them): the kernel never writes past it, and n_src[i] reports what the rule found even if that were more.  The
//         entries of a segment from n_src[i] on are not written (undefined).
// angle:  per pair (o, track entry s != r): a = C_r - X_p, b = C_s - X_p, dot = (ax bx + ay by) + az bz,
//         c = dot / (sqrt(|a|^2) sqrt(|b|^2)) in fp64, each operation rounded once (-ffp-contract=off); a zero length gives
//         weight 0; bin = the largest k in 0 .. n_bins - 1 with c <= edge[k] (0 when there is none), searched in the table the
//         host hands over; no transcendental function on the device.
// Atomics: integer atomicAdd only, results unused: the same bits for any order of the observations and of the track entries.
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int VS_BLOCK = 256;
constexpr int VS_WAVES = VS_BLOCK / 64;
constexpr int VS_BATCH = 1024;                                   // reference images per launch on the global path
constexpr int VS_LDS_RESERVED = 1024;                            // bytes kept for the kernel's static LDS
constexpr int VS_LDS_IMAGES = (160 * 1024 - VS_LDS_RESERVED) / 4;   // counters a workgroup's dynamic LDS holds
constexpr int VS_MAX_PAIRS = 1 << 22;                            // sum of the track lengths of an image, exclusive
static_assert(D3D_VIEW_SELECT_MAX_BLOCKS * 4 * sizeof(double) <= 64 * 1024, "the block table must fit in static LDS");

__global__ __launch_bounds__(VS_BLOCK) void view_select_blocks_kernel(const double* __restrict__ xyz, const long long* __restrict__ trk_offset,
                                                                      const int* __restrict__ trk_image, long n_pts, long n_trk, long p_first,
                                                                      int n_img, const double* __restrict__ blocks, int n_blocks,
                                                                      unsigned char* __restrict__ mask) {
    __shared__ double table[D3D_VIEW_SELECT_MAX_BLOCKS * 4];
    for (int t = threadIdx.x; t < 4 * n_blocks; t += VS_BLOCK) table[t] = blocks[t];
    __syncthreads();
    const long p = p_first + (long)blockIdx.x * VS_BLOCK + threadIdx.x;
    if (p >= n_pts) return;
    const double x = xyz[3 * p], y = xyz[3 * p + 1];
    long long t0 = trk_offset[p], t1 = trk_offset[p + 1];
    if (t0 < 0) t0 = 0;   // (never true for a CSR offset: a guard on the loads)
    if (t1 > n_trk) t1 = n_trk;
    for (int b = 0; b < n_blocks; ++b) {
        if (!(table[4 * b] < x && x < table[4 * b + 1] && table[4 * b + 2] < y && y < table[4 * b + 3])) continue;
        unsigned char* row = mask + (size_t)b * (size_t)n_img;
        for (long long t = t0; t < t1; ++t) {
            const int k = trk_image[t];
            if (k >= 0 && k < n_img) row[k] = 1;
        }
    }
}

template <bool LDS>
__device__ __forceinline__ unsigned vs_read(const unsigned* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the L1: the row was written by atomics
}

// The weight of the angle at X between the directions to A and to B (the header's rule).
__device__ __forceinline__ unsigned vs_weight(double ax, double ay, double az, double la, const double* __restrict__ cs,
                                              double px, double py, double pz, const double* __restrict__ edge,
                                              const unsigned* __restrict__ weight, int n_bins) {
    const double bx = cs[0] - px, by = cs[1] - py, bz = cs[2] - pz;
    const double lb = (bx * bx + by * by) + bz * bz;
    if (la == 0.0 || lb == 0.0) return 0u;
    const double dot = (ax * bx + ay * by) + az * bz;
    const double c = dot / (sqrt(la) * sqrt(lb));
    int lo = 0, hi = n_bins;   // edge does not increase: the k with c <= edge[k] are 0 .. lo - 1
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (c <= edge[mid]) lo = mid + 1;
        else hi = mid;
    }
    return weight[lo > 0 ? lo - 1 : 0];
}

template <bool LDS, bool ANGLE>
__global__ __launch_bounds__(VS_BLOCK) void view_select_rows_kernel(const long long* __restrict__ img_offset, const int* __restrict__ obs_point,
                                                                    long n_obs, const long long* __restrict__ trk_offset,
                                                                    const int* __restrict__ trk_image, long n_pts, long n_trk, int n_img,
                                                                    const int* __restrict__ refs, const double* __restrict__ centers,
                                                                    const double* __restrict__ xyz, const double* __restrict__ edge,
                                                                    const unsigned* __restrict__ weight, int n_bins,
                                                                    unsigned* __restrict__ scratch, const long long* __restrict__ seg_offset,
                                                                    int* __restrict__ seen, unsigned* __restrict__ maxv, int* __restrict__ n_src,
                                                                    int* __restrict__ src, unsigned* __restrict__ score,
                                                                    unsigned* __restrict__ count) {
    extern __shared__ unsigned vs_dyn[];
    __shared__ int scan_lds[VS_WAVES];
    __shared__ unsigned red_max[VS_WAVES];
    __shared__ int red_seen[VS_WAVES];
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    constexpr int ROWS = ANGLE ? 2 : 1;
    unsigned* row_c = LDS ? vs_dyn : scratch + (size_t)i * ROWS * (size_t)n_img;
    unsigned* row_s = row_c + (ANGLE ? n_img : 0);
    const int r = refs[i];
    const bool known = r >= 0 && r < n_img;   // (the host checks refs: a guard on the loads)
    if (LDS) {
        for (int s = tid; s < ROWS * n_img; s += VS_BLOCK) row_c[s] = 0u;
        __syncthreads();
    }
    if (known) {
        long long o0 = img_offset[r], o1 = img_offset[r + 1];
        if (o0 < 0) o0 = 0;
        if (o1 > n_obs) o1 = n_obs;
        double cx = 0.0, cy = 0.0, cz = 0.0;
        if (ANGLE) {
            cx = centers[3 * (size_t)r];
            cy = centers[3 * (size_t)r + 1];
            cz = centers[3 * (size_t)r + 2];
        }
        for (long long o = o0 + tid; o < o1; o += VS_BLOCK) {
            const int p = obs_point[o];
            if (p < 0 || p >= n_pts) continue;
            long long t0 = trk_offset[p], t1 = trk_offset[p + 1];
            if (t0 < 0) t0 = 0;
            if (t1 > n_trk) t1 = n_trk;
            double px = 0.0, py = 0.0, pz = 0.0, ax = 0.0, ay = 0.0, az = 0.0, la = 0.0;
            if (ANGLE) {
                px = xyz[3 * (size_t)p];
                py = xyz[3 * (size_t)p + 1];
                pz = xyz[3 * (size_t)p + 2];
                ax = cx - px;
                ay = cy - py;
                az = cz - pz;
                la = (ax * ax + ay * ay) + az * az;
            }
            for (long long t = t0; t < t1; ++t) {
                const int s = trk_image[t];
                if (s < 0 || s >= n_img) continue;
                atomicAdd(row_c + s, 1u);
                if (ANGLE && s != r) {
                    const unsigned w = vs_weight(ax, ay, az, la, centers + 3 * (size_t)s, px, py, pz, edge, weight, n_bins);
                    if (w != 0u) atomicAdd(row_s + s, w);
                }
            }
        }
    }
    __syncthreads();   // waits for the workgroup's atomics, LDS or global
    // seen and max over the columns but the row's own
    unsigned m = 0u;
    int sn = 0;
    for (int s = tid; s < n_img; s += VS_BLOCK) {
        if (s == r) continue;
        const unsigned c = vs_read<LDS>(row_c + s);
        const unsigned v = ANGLE ? vs_read<LDS>(row_s + s) : c;
        sn += c > 0u ? 1 : 0;
        m = max(m, v);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
        sn += __shfl_xor(sn, d, 64);
    }
    if ((tid & 63) == 0) {
        red_max[tid >> 6] = m;
        red_seen[tid >> 6] = sn;
    }
    __syncthreads();
    m = 0u;
    sn = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; ++w) {
        m = max(m, red_max[w]);
        sn += red_seen[w];
    }
    // the sources, in ascending s
    const long long seg0 = seg_offset[i], room = seg_offset[i + 1] - seg0;
    int found = 0;
    for (int base = 0; base < n_img; base += VS_BLOCK) {   // the same trip count for every lane: the scan holds barriers
        const int s = base + tid;
        unsigned c = 0u, v = 0u;
        int is = 0;
        if (s < n_img && s != r) {
            c = vs_read<LDS>(row_c + s);
            v = ANGLE ? vs_read<LDS>(row_s + s) : c;
            is = c > 10u && 10ull * (unsigned long long)v > (unsigned long long)m ? 1 : 0;
        }
        int total;
        const int at = found + block_exclusive(is, scan_lds, &total);
        if (is && at < room) {
            src[seg0 + at] = s;
            score[seg0 + at] = v;
            count[seg0 + at] = c;
        }
        found += total;
    }
    if (tid == 0) {
        seen[i] = sn;
        maxv[i] = m;
        n_src[i] = found;
    }
}

static size_t vs_scratch(long long n_ref, int n_img, int rows, long long lds_images) {
    if ((long long)rows * n_img <= lds_images) return 256;   // the LDS path: no row in device memory
    const long long batch = n_ref < VS_BATCH ? (n_ref > 0 ? n_ref : 1) : VS_BATCH;
    return align256((size_t)batch * (size_t)rows * (size_t)n_img * sizeof(unsigned));
}

template <bool LDS, bool ANGLE>
static int vs_launch(int n_rows, int lds_bytes, hipStream_t st, const long long* img_offset, const int* obs_point, long n_obs,
                     const long long* trk_offset, const int* trk_image, long n_pts, long n_trk, int n_img, const int* refs,
                     const double* centers, const double* xyz, const double* edge, const unsigned* weight, int n_bins, unsigned* scratch,
                     const long long* seg_offset, int* seen, unsigned* maxv, int* n_src, int* src, unsigned* score, unsigned* count) {
    auto kern = view_select_rows_kernel<LDS, ANGLE>;
    if (LDS) {
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_bytes);
        if (rc != D3D_OK) return rc;
    }
    hipLaunchKernelGGL(kern, dim3(n_rows), dim3(VS_BLOCK), LDS ? lds_bytes : 0, st, img_offset, obs_point, n_obs, trk_offset, trk_image, n_pts,
                       n_trk, n_img, refs, centers, xyz, edge, weight, n_bins, scratch, seg_offset, seen, maxv, n_src, src, score, count);
    D3D_LAUNCH_CHECK("view_select_rows_kernel launch");
    return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_view_select_lds_images(void) { return VS_LDS_IMAGES; }

extern "C" size_t d3d_view_select_scratch_bytes(long long n_ref, int n_img, int mode, long long lds_images) {
    if (!count_ok(n_ref) || n_img < 0 || (mode != 0 && mode != 1) || lds_images < 0 || lds_images > VS_LDS_IMAGES) return 0;
    return vs_scratch(n_ref, n_img, mode ? 2 : 1, lds_images);
}

extern "C" int d3d_view_select_blocks(const double* xyz, const long long* trk_offset, const int* trk_image, long long n_pts, long long n_trk,
                                      long long p_first, int n_img, const double* blocks, int n_blocks, unsigned char* mask,
                                      d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_pts) && count_ok(n_trk), "n_pts=%lld n_trk=%lld (0 .. 2^31 - 1)", n_pts, n_trk);
    D3D_REQUIRE(p_first >= 0 && p_first <= n_pts, "p_first=%lld with %lld points", p_first, n_pts);
    D3D_REQUIRE(n_img >= 0 && n_blocks >= 0 && n_blocks <= D3D_VIEW_SELECT_MAX_BLOCKS, "n_img=%d n_blocks=%d (at most %d blocks)", n_img,
                n_blocks, D3D_VIEW_SELECT_MAX_BLOCKS);
    const size_t cells = (size_t)n_blocks * (size_t)n_img;
    if (cells == 0) return D3D_OK;
    D3D_REQUIRE(blocks && mask, "null pointer (blocks, mask)");
    D3D_REQUIRE((xyz && trk_offset) || n_pts == 0, "null pointer (xyz, trk_offset) with %lld points", n_pts);
    D3D_REQUIRE(trk_image || n_trk == 0, "null pointer (trk_image) with %lld track entries", n_trk);
    D3D_REQUIRE((uintptr_t)xyz % 8 == 0 && (uintptr_t)trk_offset % 8 == 0 && (uintptr_t)trk_image % 4 == 0 && (uintptr_t)blocks % 8 == 0,
                "xyz, trk_offset and blocks must be 8-byte aligned and trk_image 4-byte aligned");
    const SearchRange R[5] = {{xyz, (size_t)n_pts * 24}, {trk_offset, (size_t)(n_pts + 1) * 8}, {trk_image, (size_t)n_trk * 4},
                              {blocks, (size_t)n_blocks * 32}, {mask, cells}};
    D3D_REQUIRE(search_apart(R, 5), "xyz, trk_offset, trk_image, blocks and mask must not alias");
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(mask, 0, cells, st), "view select: clear mask");
    if (rc != D3D_OK) return rc;
    const long long n = n_pts - p_first;
    if (n == 0) return D3D_OK;
    hipLaunchKernelGGL(view_select_blocks_kernel, dim3(ceil_div(n, VS_BLOCK)), dim3(VS_BLOCK), 0, st, xyz, trk_offset, trk_image, (long)n_pts,
                       (long)n_trk, (long)p_first, n_img, blocks, n_blocks, mask);
    D3D_LAUNCH_CHECK("view_select_blocks_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_view_select_rows(const long long* img_offset, const int* obs_point, long long n_obs, const long long* trk_offset,
                                    const int* trk_image, long long n_pts, long long n_trk, int n_img, const int* refs, long long n_ref,
                                    int mode, const double* centers, const double* xyz, const double* edge, const unsigned* weight,
                                    int n_bins, long long lds_images, void* scratch, size_t scratch_bytes, const long long* seg_offset,
                                    long long n_seg, int* seen, unsigned* maxv, int* n_src, int* src, unsigned* score, unsigned* count,
                                    d3d_stream_t stream) {
    D3D_REQUIRE(count_ok(n_obs) && count_ok(n_pts) && count_ok(n_trk) && count_ok(n_ref) && count_ok(n_seg),
                "n_obs=%lld n_pts=%lld n_trk=%lld n_ref=%lld n_seg=%lld (0 .. 2^31 - 1)", n_obs, n_pts, n_trk, n_ref, n_seg);
    D3D_REQUIRE(n_img >= 1, "n_img=%d (at least 1)", n_img);
    D3D_REQUIRE(mode == 0 || mode == 1, "mode=%d (0 points, 1 angle)", mode);
    D3D_REQUIRE(lds_images >= 0 && lds_images <= VS_LDS_IMAGES, "lds_images=%lld (0 .. %d)", lds_images, VS_LDS_IMAGES);
    if (n_ref == 0) return D3D_OK;
    const int rows = mode ? 2 : 1;
    D3D_REQUIRE(img_offset && trk_offset && refs && scratch && seg_offset && seen && maxv && n_src,
                "null pointer (img_offset, trk_offset, refs, scratch, seg_offset, seen, maxv, n_src)");
    D3D_REQUIRE(obs_point || n_obs == 0, "null pointer (obs_point) with %lld observations", n_obs);
    D3D_REQUIRE(trk_image || n_trk == 0, "null pointer (trk_image) with %lld track entries", n_trk);
    D3D_REQUIRE((src && score && count) || n_seg == 0, "null pointer (src, score, count) with %lld slots", n_seg);
    D3D_REQUIRE(mode == 0 || (centers && edge && weight && n_bins >= 1 && (xyz || n_pts == 0)),
                "angle mode needs centers, xyz, edge, weight and n_bins >= 1 (got %d)", n_bins);
    const uintptr_t a8 = (uintptr_t)img_offset | (uintptr_t)trk_offset | (uintptr_t)seg_offset | (uintptr_t)centers | (uintptr_t)xyz |
                         (uintptr_t)edge;
    const uintptr_t a4 = (uintptr_t)obs_point | (uintptr_t)trk_image | (uintptr_t)refs | (uintptr_t)weight | (uintptr_t)scratch |
                         (uintptr_t)seen | (uintptr_t)maxv | (uintptr_t)n_src | (uintptr_t)src | (uintptr_t)score | (uintptr_t)count;
    D3D_REQUIRE(a8 % 8 == 0 && a4 % 4 == 0, "the 64-bit buffers must be 8-byte aligned and the 32-bit ones 4-byte aligned");
    const size_t need = vs_scratch(n_ref, n_img, rows, lds_images);
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_view_select_scratch_bytes)", scratch_bytes, need);
    const size_t nr = (size_t)n_ref, ns = (size_t)n_seg, nb = mode ? (size_t)n_bins : 0;
    const SearchRange R[17] = {{img_offset, ((size_t)n_img + 1) * 8}, {obs_point, (size_t)n_obs * 4}, {trk_offset, (size_t)(n_pts + 1) * 8},
                               {trk_image, (size_t)n_trk * 4}, {refs, nr * 4}, {mode ? centers : nullptr, (size_t)n_img * 24},
                               {mode ? xyz : nullptr, (size_t)n_pts * 24}, {edge, nb * 8}, {weight, nb * 4}, {scratch, scratch_bytes},
                               {seg_offset, (nr + 1) * 8}, {seen, nr * 4}, {maxv, nr * 4}, {n_src, nr * 4}, {src, ns * 4}, {score, ns * 4},
                               {count, ns * 4}};
    D3D_REQUIRE(search_apart(R, 17), "the buffers of d3d_view_select_rows must not alias");
    hipStream_t st = (hipStream_t)stream;
    const bool lds = (long long)rows * n_img <= lds_images;
    const int lds_bytes = rows * n_img * (int)sizeof(unsigned);
    const long long batch = lds ? n_ref : VS_BATCH;
    for (long long base = 0; base < n_ref; base += batch) {
        const int n_rows = (int)(n_ref - base < batch ? n_ref - base : batch);
        int rc = D3D_OK;
        if (!lds) {
            rc = hip_status(hipMemsetAsync(scratch, 0, (size_t)n_rows * rows * (size_t)n_img * sizeof(unsigned), st), "view select: clear rows");
            if (rc != D3D_OK) return rc;
        }
#define VS_ARGS                                                                                                                            \
    n_rows, lds_bytes, st, img_offset, obs_point, (long)n_obs, trk_offset, trk_image, (long)n_pts, (long)n_trk, n_img, refs + base, centers, \
        xyz, edge, weight, n_bins, (unsigned*)scratch, seg_offset + base, seen + base, maxv + base, n_src + base, src, score, count
        if (lds) rc = mode ? vs_launch<true, true>(VS_ARGS) : vs_launch<true, false>(VS_ARGS);
        else rc = mode ? vs_launch<false, true>(VS_ARGS) : vs_launch<false, false>(VS_ARGS);
#undef VS_ARGS
        if (rc != D3D_OK) return rc;
    }
    return D3D_OK;
}
