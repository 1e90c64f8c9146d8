// True orthophoto on the DSM: the semantics are this project's (deep3d_aerial_amd/ortho.py states them,
// include/deep3d_planesweep.h too).  The reference has no orthophoto step.
//
// Cell (i, j) of the W x H grid is X = (x_min + (j + 0.5) ux, y_max - (i + 0.5) uy, h), h the DSM height in fp64; a non-finite
// h is an empty cell.  Per view, in fp64 with no contraction: p = R X + t, q = K p (rows summed left to right), u = q0 / q2,
// v = q1 / q2.  The view is a candidate when p2 > 0, q2 > 0, 0 <= u <= W-1, 0 <= v <= H-1, the depth D at
// (floor(v + 0.5), floor(u + 0.5)) is finite and > 0, and p2 <= D (1 + tol).  Its score s = (dx^2 + dy^2) / dz^2,
// (dx, dy, dz) = X - C (C = -R^T t); a non-finite s rejects the view.  key = (bits(fp32(s)) << 32) | id, the smallest wins.
//
// select: per (16 x 16 tile, 64 views) one wave: the tile's finite height range (shuffle reduction), the 8 corners of the
//         tile's box projected with a 1-pixel margin, one ballot -> one 64-bit word of the tile's candidate mask.  A view
//         with a corner at p2 <= 0 or q2 <= 0 stays a candidate: culling only skips work.
//         Then one workgroup per tile walks the set bits (wave-uniform); each lane projects its cell, gathers D and keeps
//         its best key in registers; one min-merge into `key` at the end.
// colorize: per cell, the winner's (u, v) again and a bilinear sample of its RGBA8 copy (geom_blend; (u, v) is inside the image,
//           so the tap indices need no clamp from below).
// No atomics: a key is a minimum, so any batching or split of the views gives the same bits.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int ORTHO_TILE = 16;
constexpr int ORTHO_BLOCK = ORTHO_TILE * ORTHO_TILE;
constexpr long long ORTHO_EMPTY = 0x7fffffffffffffffll;
static_assert(sizeof(d3d_ortho_view_t) == 224, "d3d_ortho_view_t: the layout deep3d_aerial_amd/ortho.py fills");

struct OrthoGrid {
    double x_min, y_max, ux, uy;
    int W, H;
};

__device__ __forceinline__ double ortho_x(const OrthoGrid& g, int j) { return g.x_min + ((double)j + 0.5) * g.ux; }
__device__ __forceinline__ double ortho_y(const OrthoGrid& g, int i) { return g.y_max - ((double)i + 0.5) * g.uy; }

// One wave per (tile, word): lane l decides view 64 word + l.  mask [n_tiles, n_words] uint64.
__global__ __launch_bounds__(ORTHO_BLOCK) void ortho_cull_kernel(const float* __restrict__ height, OrthoGrid g, int tiles_x, int n_tiles,
                                                                 const d3d_ortho_view_t* __restrict__ views, int n_views, int n_words,
                                                                 unsigned long long* __restrict__ mask) {
    const long wave = ((long)blockIdx.x * ORTHO_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= (long)n_tiles * n_words) return;   // whole waves: n_tiles * n_words waves in all
    const int tile = (int)(wave / n_words), word = (int)(wave - (long)tile * n_words);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int i0 = ty * ORTHO_TILE, j0 = tx * ORTHO_TILE;
    const int i1 = min(i0 + ORTHO_TILE, g.H) - 1, j1 = min(j0 + ORTHO_TILE, g.W) - 1;
    // the tile's finite height range: 4 cells per lane
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int k = 0; k < ORTHO_BLOCK / 64; ++k) {
        const int c = k * 64 + lane;
        const int i = i0 + (c >> 4), j = j0 + (c & 15);
        if (i <= i1 && j <= j1) {
            const float h = height[(long)i * g.W + j];
            if (isfinite(h)) {
                lo = fminf(lo, h);
                hi = fmaxf(hi, h);
            }
        }
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int vi = word * 64 + lane;
    bool cand = false;
    if (vi < n_views && lo <= hi) {
        const d3d_ortho_view_t& V = views[vi];
        const double xs[2] = {ortho_x(g, j0), ortho_x(g, j1)}, ys[2] = {ortho_y(g, i0), ortho_y(g, i1)}, zs[2] = {(double)lo, (double)hi};
        double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
        bool keep = false;   // a corner behind the view (or a non-finite projection): no bound, the view stays
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const GeomPq r = geom_project(V, xs[k & 1], ys[(k >> 1) & 1], zs[k >> 2]);
            if (!(r.p2 > 0.0 && r.q2 > 0.0)) {
                keep = true;
                continue;
            }
            const double u = r.q0 / r.q2, v = r.q1 / r.q2;
            if (!(isfinite(u) && isfinite(v))) {
                keep = true;
                continue;
            }
            umin = fmin(umin, u);
            umax = fmax(umax, u);
            vmin = fmin(vmin, v);
            vmax = fmax(vmax, v);
        }
        // all corners in front: the box projects inside the hull of its corners (a projective map keeps convexity where q2 > 0)
        cand = keep || !(umax < -1.0 || umin > (double)V.W || vmax < -1.0 || vmin > (double)V.H);
    }
    const unsigned long long bits = __ballot(cand);
    if (lane == 0) mask[wave] = bits;
}

__global__ __launch_bounds__(ORTHO_BLOCK) void ortho_select_kernel(const float* __restrict__ height, OrthoGrid g, int tiles_x,
                                                                   const d3d_ortho_view_t* __restrict__ views, int n_words, double tol1,
                                                                   const unsigned long long* __restrict__ mask,
                                                                   long long* __restrict__ key) {
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int i = ty * ORTHO_TILE + (threadIdx.x >> 4), j = tx * ORTHO_TILE + (threadIdx.x & 15);
    const bool in = i < g.H && j < g.W;
    const long c = (long)i * g.W + j;
    const float h = in ? height[c] : 0.0f;
    const bool live = in && isfinite(h);
    const double X0 = ortho_x(g, j), X1 = ortho_y(g, i), X2 = (double)h;
    long long best = live ? key[c] : ORTHO_EMPTY;
    const unsigned long long* m = mask + (long)tile * n_words;
    for (int w = 0; w < n_words; ++w) {
        unsigned long long bits = m[w];
        while (bits) {
            const int vi = __builtin_amdgcn_readfirstlane(w * 64 + __builtin_ctzll(bits));
            bits &= bits - 1;
            if (!live) continue;
            const d3d_ortho_view_t& V = views[vi];
            double u, v, p2;
            if (!geom_uv(V, X0, X1, X2, &u, &v, &p2)) continue;
            const float D = geom_depth_at(V, u, v);
            if (!(isfinite(D) && D > 0.0f && p2 <= (double)D * tol1)) continue;
            const double dx = X0 - V.C[0], dy = X1 - V.C[1], dz = X2 - V.C[2];
            const double s = (dx * dx + dy * dy) / (dz * dz);
            if (!isfinite(s)) continue;
            const long long k = geom_view_key(s, V.id);
            best = k < best ? k : best;
        }
    }
    if (live) key[c] = best;
}

__global__ __launch_bounds__(ORTHO_BLOCK) void ortho_colorize_kernel(const float* __restrict__ height, OrthoGrid g,
                                                                     const long long* __restrict__ key,
                                                                     const d3d_ortho_view_t* __restrict__ views, int n_views,
                                                                     unsigned* __restrict__ rgba, int* __restrict__ view_out) {
    const long c = (long)blockIdx.x * ORTHO_BLOCK + threadIdx.x;
    if (c >= (long)g.W * g.H) return;
    const long long k = key[c];
    if (k == ORTHO_EMPTY) return;
    const int id = geom_key_id(k);
    int slot = -1;
    for (int q = 0; q < n_views; ++q)   // wave-uniform loop over this call's records
        if (views[q].id == id) slot = q;
    if (slot < 0) return;
    const float h = height[c];
    if (!isfinite(h)) return;
    const int i = (int)(c / g.W), j = (int)(c - (long)i * g.W);
    const d3d_ortho_view_t& V = views[slot];
    double u, v, p2;
    if (!geom_uv(V, ortho_x(g, j), ortho_y(g, i), (double)h, &u, &v, &p2)) return;   // the key came from another raster
    const double fu = floor(u), fv = floor(v);
    const double fx = u - fu, fy = v - fv;
    const int x0 = min((int)fu, V.W - 1), y0 = min((int)fv, V.H - 1);
    const int x1 = min(x0 + 1, V.W - 1), y1 = min(y0 + 1, V.H - 1);
    const unsigned t00 = V.rgba[(long)y0 * V.W + x0], t10 = V.rgba[(long)y0 * V.W + x1];
    const unsigned t01 = V.rgba[(long)y1 * V.W + x0], t11 = V.rgba[(long)y1 * V.W + x1];
    double s[3];
    geom_blend(t00, t10, t01, t11, fx, fy, s);
    unsigned out = 255u << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double r = fmin(fmax(floor(s[ch] + 0.5), 0.0), 255.0);
        out |= (unsigned)r << (8 * ch);
    }
    rgba[c] = out;
    view_out[c] = id;
}

static bool ortho_dims_ok(int W, int H, int n_views) {
    return W >= 1 && H >= 1 && (long long)W * H < (1ll << 31) && n_views >= 0 && n_views < (1 << 20);
}

static long long ortho_tiles(int W, int H) { return (long long)ceil_div(W, ORTHO_TILE) * ceil_div(H, ORTHO_TILE); }

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_ortho_scratch_bytes(int W, int H, int n_views) {
    if (!ortho_dims_ok(W, H, n_views)) return 0;
    return (size_t)ortho_tiles(W, H) * ceil_div(n_views, 64) * 8;
}

#define ORTHO_CHECK_GRID()                                                                                                             \
    D3D_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "raster %d x %d: size must be >= 1 and W * H < 2^31", W, H);       \
    D3D_REQUIRE(std::isfinite(unit_x) && std::isfinite(unit_y) && unit_x > 0.0 && unit_y > 0.0, "unit (%g, %g) must be finite and > 0", \
                unit_x, unit_y);                                                                                                       \
    D3D_REQUIRE(std::isfinite(x_min) && std::isfinite(y_max), "border (x_min %g, y_max %g) must be finite", x_min, y_max)

extern "C" int d3d_ortho_select(const float* height, double x_min, double y_max, double unit_x, double unit_y, int W, int H,
                                const d3d_ortho_view_t* views, int n_views, double depth_tolerance, void* scratch, size_t scratch_bytes,
                                long long* key, d3d_stream_t stream) {
    D3D_REQUIRE(height && key, "null pointer (height, key)");
    ORTHO_CHECK_GRID();
    D3D_REQUIRE(n_views >= 0 && n_views < (1 << 20), "n_views=%d (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    D3D_REQUIRE(std::isfinite(depth_tolerance) && depth_tolerance >= 0.0, "depth_tolerance=%g must be finite and >= 0", depth_tolerance);
    if (n_views == 0) return D3D_OK;
    const size_t need = d3d_ortho_scratch_bytes(W, H, n_views);
    D3D_REQUIRE(scratch, "null pointer (scratch)");
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_ortho_scratch_bytes)", scratch_bytes, need);
    const OrthoGrid g = {x_min, y_max, unit_x, unit_y, W, H};
    const int tiles_x = ceil_div(W, ORTHO_TILE);
    const long long n_tiles = ortho_tiles(W, H);
    const int n_words = ceil_div(n_views, 64);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* mask = (unsigned long long*)scratch;
    const long long waves = n_tiles * n_words;
    D3D_REQUIRE(waves < (1ll << 31) / 4, "%lld tiles x %d mask words: too many", n_tiles, n_words);
    hipLaunchKernelGGL(ortho_cull_kernel, dim3(ceil_div(waves, ORTHO_BLOCK / 64)), dim3(ORTHO_BLOCK), 0, st, height, g, tiles_x,
                       (int)n_tiles, views, n_views, n_words, mask);
    D3D_LAUNCH_CHECK("ortho_cull_kernel launch");
    hipLaunchKernelGGL(ortho_select_kernel, dim3((unsigned)n_tiles), dim3(ORTHO_BLOCK), 0, st, height, g, tiles_x, views, n_words,
                       1.0 + depth_tolerance, mask, key);
    D3D_LAUNCH_CHECK("ortho_select_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_ortho_colorize(const float* height, double x_min, double y_max, double unit_x, double unit_y, int W, int H,
                                  const long long* key, const d3d_ortho_view_t* views, int n_views, unsigned int* rgba, int* view_out,
                                  d3d_stream_t stream) {
    D3D_REQUIRE(height && key && rgba && view_out, "null pointer (height, key, rgba, view_out)");
    ORTHO_CHECK_GRID();
    D3D_REQUIRE(n_views >= 0 && n_views < (1 << 20), "n_views=%d (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    if (n_views == 0) return D3D_OK;
    const OrthoGrid g = {x_min, y_max, unit_x, unit_y, W, H};
    hipLaunchKernelGGL(ortho_colorize_kernel, dim3(ceil_div((long)W * H, ORTHO_BLOCK)), dim3(ORTHO_BLOCK), 0, (hipStream_t)stream, height, g,
                       key, views, n_views, rgba, view_out);
    D3D_LAUNCH_CHECK("ortho_colorize_kernel launch");
    return D3D_OK;
}
