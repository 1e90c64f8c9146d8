// Texturing the surface mesh from the views: the semantics are this project's (deep3d_aerial_amd/texture.py
// states them, include/deep3d_planesweep.h too); they do not claim to match OpenMVS's TextureMesh.
//
// select:    per (block of 256 faces, views) one wave: the fp32 box of the block's corners, its 8 corners projected per view with
//            a 1-pixel margin, one ballot per 64 views -> the block's candidate mask (ortho.hip's tile cull: a corner at p2 <= 0
//            keeps the view; culling only skips work).  Then one workgroup per block: each lane owns a face, walks the set bits
//            (wave-uniform), runs the candidate tests in fp64 and keeps its best key in registers; one min-merge into `key`.
// charts:    (edge key, face) pairs sorted by (edge, winner) by the caller; hooking over adjacent pairs of equal edge and winner
//            (geom_hook) and pointer jumping until a hooking launch changes nothing, as mesh_clean.hip's components.  The fixed
//            point is the smallest face index; a scan numbers the roots.
// rects:     one lane per face projects its corners in its winner's view; integer atomicMin / atomicMax into its chart's rect,
//            folded over the wave when every lane of it has the same chart.
// fill:      one wave per (chart, band of rows): coalesced 4-byte copies of the view's RGBA8 rows into the atlas.
// empty:     texels no fill wrote (alpha 0) get the empty colour.
// texcoords: one lane per face.
// No float atomics; the integer atomics are min / max, whose results do not depend on the order the lanes run in.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"
#include "texture_shared.h"

namespace d3d {

constexpr long long TX_EDGE_NONE = 0x7fffffffffffffffll;

// ---------------------------------------------------------------------------------------------------------------------------
// select
// ---------------------------------------------------------------------------------------------------------------------------
// One wave per block of TX_BLOCK faces; lane l decides views 64 w + l.  mask [n_blocks, n_words] uint64.
__global__ __launch_bounds__(TX_BLOCK) void tx_cull_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                           long m, long n_blocks, const d3d_ortho_view_t* __restrict__ views, int n_views,
                                                           int n_words, unsigned long long* __restrict__ mask) {
    const long block = ((long)blockIdx.x * TX_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (block >= n_blocks) return;   // whole waves
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < TX_BLOCK / 64; ++k) {
        const long f = block * TX_BLOCK + k * 64 + lane;
        if (f >= m) break;
        int ia, ib, ic;
        if (!geom_face<false>(faces, f, n, &ia, &ib, &ic)) continue;
        const int idx[3] = {ia, ib, ic};
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float x = vertices[3l * idx[q] + ax];
                lo[ax] = fminf(lo[ax], x);
                hi[ax] = fmaxf(hi[ax], x);
            }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = wave_min(lo[ax]);
        hi[ax] = wave_max(hi[ax]);
    }
    const bool any = lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
    for (int w = 0; w < n_words; ++w) {
        const int vi = w * 64 + lane;
        bool cand = false;
        if (vi < n_views && any) {
            const d3d_ortho_view_t& V = views[vi];
            double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
            bool keep = false;   // a corner behind the view (or a non-finite projection): no bound, the view stays
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const GeomPq r = geom_project(V, (double)(k & 1 ? hi[0] : lo[0]), (double)(k & 2 ? hi[1] : lo[1]),
                                                (double)(k & 4 ? hi[2] : lo[2]));
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
            cand = keep || !(umax < -1.0 || umin > (double)V.W || vmax < -1.0 || vmin > (double)V.H);
        }
        const unsigned long long bits = __ballot(cand);
        if (lane == 0) mask[block * n_words + w] = bits;
    }
}

__global__ __launch_bounds__(TX_BLOCK) void tx_select_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                             long m, const d3d_ortho_view_t* __restrict__ views, int n_words, double tol1,
                                                             const unsigned long long* __restrict__ mask, long long* __restrict__ key) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    TxFrame T;
    const bool live = tx_frame(vertices, faces, f, m, n, &T);
    long long best = live ? key[f] : TX_EMPTY;
    const unsigned long long* mk = mask + (long)blockIdx.x * n_words;
    for (int w = 0; w < n_words; ++w) {
        unsigned long long bits = mk[w];
        while (bits) {
            const int vi = __builtin_amdgcn_readfirstlane(w * 64 + __builtin_ctzll(bits));
            bits &= bits - 1;
            long long k;
            if (live && tx_view_key(views[vi], T, tol1, &k)) best = k < best ? k : best;
        }
    }
    if (live) key[f] = best;
}

// ---------------------------------------------------------------------------------------------------------------------------
// charts
// ---------------------------------------------------------------------------------------------------------------------------
// edge_key [3 m]: slot 3 f + k holds the k-th distinct edge of face f as min(i, j) * n + max(i, j) when f has a winner, else
// TX_EDGE_NONE (geom_face_edges: (a,b) (b,c) (c,a) with unequal ends, each unordered pair once).
__global__ __launch_bounds__(TX_BLOCK) void tx_edges_kernel(const int* __restrict__ faces, long m, long long n, const long long* __restrict__ key,
                                                            long long* __restrict__ edge_key) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    long long e[3] = {TX_EDGE_NONE, TX_EDGE_NONE, TX_EDGE_NONE};
    int a, b, c;
    if (geom_face<false>(faces, f, n, &a, &b, &c) && key[f] != TX_EMPTY) {
        int x[3], y[3];
        const int ne = geom_face_edges(a, b, c, x, y);
        for (int k = 0; k < ne; ++k) e[k] = (long long)min(x[k], y[k]) * n + max(x[k], y[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) edge_key[3 * f + k] = e[k];
}

// Pairs sorted by (edge, winner): pair i joins pair i - 1 when both have the same edge and the same winner.
__global__ __launch_bounds__(TX_BLOCK) void tx_hook_kernel(const long long* __restrict__ edge_sorted, const int* __restrict__ face_sorted,
                                                           long n_pairs, const long long* __restrict__ key, int* parent, int* changed) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x + 1;
    if (i >= n_pairs) return;
    const long long e = edge_sorted[i];
    if (e == TX_EDGE_NONE || e != edge_sorted[i - 1]) return;
    const int fa = face_sorted[i], fb = face_sorted[i - 1];
    if ((unsigned)key[fa] != (unsigned)key[fb]) return;   // the winners' ids (both faces have one: their edges are listed)
    geom_hook(parent, parent[fa], parent[fb], changed);
}

__global__ __launch_bounds__(TX_BLOCK) void tx_roots_kernel(const long long* __restrict__ key, const int* __restrict__ label, long m,
                                                            int* __restrict__ root) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f < m) root[f] = key[f] != TX_EMPTY && label[f] == (int)f ? 1 : 0;
}

__global__ __launch_bounds__(TX_BLOCK) void tx_number_kernel(const long long* __restrict__ key, const int* __restrict__ label, long m,
                                                             const int* __restrict__ number, int* __restrict__ chart) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f < m) chart[f] = key[f] != TX_EMPTY ? number[label[f]] : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// rects
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TX_BLOCK) void tx_rect_init_kernel(int* __restrict__ rect, long n_charts) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= 4 * n_charts) return;
    rect[i] = (i & 3) < 2 ? INT_MAX : INT_MIN;
}

__global__ __launch_bounds__(TX_BLOCK) void tx_rects_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                            long m, const long long* __restrict__ key, const int* __restrict__ chart,
                                                            long n_charts, const d3d_ortho_view_t* __restrict__ cams, int n_cams, int pad,
                                                            int* __restrict__ rect) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int c = -1, r0 = INT_MAX, r1 = INT_MAX, r2 = INT_MIN, r3 = INT_MIN;
    TxFace F;
    if (f < m) {
        const long long k = key[f];
        c = chart[f];
        const int slot = k != TX_EMPTY && c >= 0 && c < n_charts ? tx_find(cams, n_cams, geom_key_id(k)) : -1;
        double u[3], v[3];
        if (slot >= 0 && tx_face(vertices, faces, f, n, &F) && tx_corner_uv(cams[slot], F, u, v)) {
            const d3d_ortho_view_t& V = cams[slot];
            const double umin = fmin(fmin(u[0], u[1]), u[2]), umax = fmax(fmax(u[0], u[1]), u[2]);
            const double vmin = fmin(fmin(v[0], v[1]), v[2]), vmax = fmax(fmax(v[0], v[1]), v[2]);
            r0 = (int)fmin(fmax(floor(umin) - pad, 0.0), (double)(V.W - 1));
            r1 = (int)fmin(fmax(floor(vmin) - pad, 0.0), (double)(V.H - 1));
            r2 = (int)fmax(fmin(ceil(umax) + pad, (double)(V.W - 1)), 0.0);
            r3 = (int)fmax(fmin(ceil(vmax) + pad, (double)(V.H - 1)), 0.0);
        } else {
            c = -1;
        }
    }
    const unsigned long long act = __ballot(c >= 0);
    if (!act) return;   // wave-uniform
    const int lead = __builtin_ctzll(act);
    const int c0 = __shfl(c, lead, 64);
    if (__all(c < 0 || c == c0)) {
        r0 = wave_min(r0), r1 = wave_min(r1), r2 = wave_max(r2), r3 = wave_max(r3);
        if (lane != lead) return;
    } else if (c < 0) {
        return;
    }
    int* R = rect + 4l * c;
    atomicMin(R, r0);
    atomicMin(R + 1, r1);
    atomicMax(R + 2, r2);
    atomicMax(R + 3, r3);
}

// ---------------------------------------------------------------------------------------------------------------------------
// fill, empty colour, texcoords
// ---------------------------------------------------------------------------------------------------------------------------
// table [n_charts, 8] int32: x0, y0, w, h, ox, oy, page, id.  page_row [n_pages + 1] int64: the atlas row each page starts at.
__global__ __launch_bounds__(TX_BLOCK) void tx_fill_kernel(const int* __restrict__ work, long n_work, const int* __restrict__ table,
                                                           long n_charts, const long long* __restrict__ page_row, int n_pages,
                                                           const d3d_ortho_view_t* __restrict__ views, int n_views, int P,
                                                           unsigned* __restrict__ atlas) {
    const long item = ((long)blockIdx.x * TX_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (item >= n_work) return;   // whole waves
    const int c = work[2 * item], band = work[2 * item + 1];
    if (c < 0 || c >= n_charts) return;
    const int* T = table + 8l * c;
    const int x0 = T[0], y0 = T[1], w = T[2], h = T[3], ox = T[4], oy = T[5], page = T[6];
    const int slot = tx_find(views, n_views, T[7]);
    if (slot < 0 || page < 0 || page >= n_pages) return;   // another caller's view
    const d3d_ortho_view_t& V = views[slot];
    const long long row0 = page_row[page] + oy;
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 + w > V.W || y0 + h > V.H || ox < 0 || ox + w > P || oy < 0 ||
        row0 + h > page_row[page + 1])
        return;   // texture.py builds the table; a bad row is skipped, never written out of bounds
    const int r_begin = band * TX_BAND;
    const int rows = min(TX_BAND, h - r_begin);
    if (rows <= 0) return;
    const int total = rows * w;
    for (int i = lane; i < total; i += 64) {
        const int dy = r_begin + i / w, dx = i - (i / w) * w;
        atlas[(row0 + dy) * (long long)P + ox + dx] = V.rgba[(long)(y0 + dy) * V.W + x0 + dx];
    }
}

__global__ __launch_bounds__(TX_BLOCK) void tx_empty_kernel(unsigned* __restrict__ atlas, long long n_texels, unsigned empty) {
    const long long i = (long long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= n_texels) return;
    if ((atlas[i] >> 24) == 0u) atlas[i] = empty;
}

__global__ __launch_bounds__(TX_BLOCK) void tx_texcoords_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                                long m, const long long* __restrict__ key, const int* __restrict__ chart,
                                                                const int* __restrict__ table, long n_charts,
                                                                const long long* __restrict__ page_row, int n_pages,
                                                                const d3d_ortho_view_t* __restrict__ cams, int n_cams, int P,
                                                                float* __restrict__ texcoord, int* __restrict__ texnumber) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    float st[6];
    int page = 0;
    const double h0 = (double)(page_row[1] - page_row[0]);
    const float es = (float)(1.0 / (double)P), et = (float)(1.0 - 1.0 / h0);
    for (int k = 0; k < 3; ++k) st[2 * k] = es, st[2 * k + 1] = et;
    const long long k = key[f];
    const int c = chart[f];
    TxFace F;
    if (k != TX_EMPTY && c >= 0 && c < n_charts) {
        const int* T = table + 8l * c;
        const int slot = tx_find(cams, n_cams, T[7]);
        double u[3], v[3];
        if (slot >= 0 && T[6] >= 0 && T[6] < n_pages && tx_face(vertices, faces, f, n, &F) && tx_corner_uv(cams[slot], F, u, v)) {
            page = T[6];
            const double x0 = (double)T[0], y0 = (double)T[1], ox = (double)T[4], oy = (double)T[5];
            const double hp = (double)(page_row[page + 1] - page_row[page]);
            for (int q = 0; q < 3; ++q) {
                st[2 * q] = (float)((((u[q] - x0) + ox) + 0.5) / (double)P);
                st[2 * q + 1] = (float)(1.0 - (((v[q] - y0) + oy) + 0.5) / hp);
            }
        }
    }
    for (int q = 0; q < 6; ++q) texcoord[6 * f + q] = st[q];
    texnumber[f] = page;
}

struct TxScratch {
    size_t root, number, scan, bytes;
};

static TxScratch tx_chart_layout(long long m) {
    const size_t nf = (size_t)(m > 0 ? m : 1);
    ScratchLayout L;
    TxScratch s;
    s.root = L.take(nf * 4);
    s.number = L.take(nf * 4);
    s.scan = L.take(geom_scan_bytes(m));
    s.bytes = L.bytes;
    return s;
}

static bool tx_sizes_ok(long long n, long long m) { return n >= 0 && n < (1ll << 31) && m >= 0 && 3 * m < (1ll << 31); }

int tx_cull(const float* vertices, long long n, const int* faces, long long m, const d3d_ortho_view_t* views, int n_views,
            unsigned long long* mask, hipStream_t st) {
    const long n_blocks = ceil_div(m, TX_BLOCK);
    hipLaunchKernelGGL(tx_cull_kernel, dim3(ceil_div(n_blocks, TX_BLOCK / 64)), dim3(TX_BLOCK), 0, st, vertices, n, faces, (long)m, n_blocks,
                       views, n_views, ceil_div(n_views, 64), mask);
    D3D_LAUNCH_CHECK("tx_cull_kernel launch");
    return D3D_OK;
}

}  // namespace d3d

using namespace d3d;

#define TX_CHECK_SIZES()                                                                                                           \
    D3D_REQUIRE(tx_sizes_ok(n_vertices, n_faces), "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 3 n_faces < 2^31)", n_vertices, \
                n_faces)

#define TX_CHECK_VIEWS(v, nv)                                                                                  \
    D3D_REQUIRE((nv) >= 0 && (nv) < (1 << 20), "%d views (0 .. 2^20 - 1)", (int)(nv));                          \
    D3D_REQUIRE((v) || (nv) == 0, "null pointer (views) with %d views", (int)(nv))

extern "C" size_t d3d_texture_scratch_bytes(long long n_faces, int n_views) {
    if (!tx_sizes_ok(0, n_faces) || n_views < 0 || n_views >= (1 << 20)) return 0;
    const size_t a = tx_mask_bytes(n_faces, n_views), b = tx_chart_layout(n_faces).bytes;
    return a > b ? a : b;
}

extern "C" int d3d_texture_select(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                  const d3d_ortho_view_t* views, int n_views, double depth_tolerance, void* scratch, size_t scratch_bytes,
                                  long long* key, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && (faces || n_faces == 0) && (key || n_faces == 0), "null pointer (vertices, faces, key)");
    TX_CHECK_SIZES();
    TX_CHECK_VIEWS(views, n_views);
    D3D_REQUIRE(std::isfinite(depth_tolerance) && depth_tolerance >= 0.0, "depth_tolerance=%g must be finite and >= 0", depth_tolerance);
    if (n_views == 0 || n_faces == 0) return D3D_OK;
    const size_t need = tx_mask_bytes(n_faces, n_views);
    D3D_REQUIRE(scratch, "null pointer (scratch)");
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_texture_scratch_bytes)", scratch_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long n_blocks = ceil_div(n_faces, TX_BLOCK);
    const int n_words = ceil_div(n_views, 64);
    unsigned long long* mask = (unsigned long long*)scratch;
    const int rc = tx_cull(vertices, n_vertices, faces, n_faces, views, n_views, mask, st);
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(tx_select_kernel, dim3((unsigned)n_blocks), dim3(TX_BLOCK), 0, st, vertices, n_vertices, faces, (long)n_faces, views,
                       n_words, 1.0 + depth_tolerance, mask, key);
    D3D_LAUNCH_CHECK("tx_select_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_edges(const int* faces, long long n_faces, long long n_vertices, const long long* key, long long* edge_key,
                                 d3d_stream_t stream) {
    D3D_REQUIRE((faces && key && edge_key) || n_faces == 0, "null pointer (faces, key, edge_key)");
    TX_CHECK_SIZES();
    if (n_faces == 0) return D3D_OK;
    hipLaunchKernelGGL(tx_edges_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream, faces, (long)n_faces,
                       n_vertices, key, edge_key);
    D3D_LAUNCH_CHECK("tx_edges_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_charts(const long long* edge_sorted, const int* face_sorted, long long n_pairs, const long long* key,
                                  long long n_faces, void* scratch, size_t scratch_bytes, int* label, int* chart, int* flag,
                                  long long* n_charts, int* rounds, d3d_stream_t stream) {
    D3D_REQUIRE(((edge_sorted && face_sorted) || n_pairs == 0) && ((key && label && chart) || n_faces == 0) && flag && n_charts && scratch,
                "null pointer (edge_sorted, face_sorted, key, label, chart, flag, n_charts, scratch)");
    D3D_REQUIRE(n_faces >= 0 && 3 * n_faces < (1ll << 31) && n_pairs >= 0 && n_pairs <= 3 * n_faces, "n_faces=%lld, n_pairs=%lld",
                n_faces, n_pairs);
    const TxScratch L = tx_chart_layout(n_faces);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed (d3d_texture_scratch_bytes)", scratch_bytes, L.bytes);
    hipStream_t st = (hipStream_t)stream;
    const long m = (long)n_faces;
    int r = 0;
    int rc = geom_iota(label, m, st);
    if (rc != D3D_OK) return rc;
    while (n_pairs > 1) {
        rc = hip_status(hipMemsetAsync(flag, 0, 4, st), "texture charts: clear flag");
        if (rc != D3D_OK) return rc;
        hipLaunchKernelGGL(tx_hook_kernel, dim3(ceil_div(n_pairs - 1, TX_BLOCK)), dim3(TX_BLOCK), 0, st, edge_sorted, face_sorted,
                           (long)n_pairs, key, label, flag);
        D3D_LAUNCH_CHECK("tx_hook_kernel launch");
        ++r;
        int h = 0;
        rc = hip_status(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st), "texture charts: read flag");
        if (rc != D3D_OK) return rc;
        rc = hip_status(hipStreamSynchronize(st), "texture charts: sync");
        if (rc != D3D_OK) return rc;
        if (!h) break;
        rc = geom_jump(label, m, st);
        if (rc != D3D_OK) return rc;
    }
    if (rounds) *rounds = r;
    char* w = (char*)scratch;
    int *root = (int*)(w + L.root), *number = (int*)(w + L.number);
    if (m > 0) {
        hipLaunchKernelGGL(tx_roots_kernel, dim3(ceil_div(m, TX_BLOCK)), dim3(TX_BLOCK), 0, st, key, label, m, root);
        D3D_LAUNCH_CHECK("tx_roots_kernel launch");
    }
    rc = geom_scan(root, number, m, w + L.scan, n_charts, st);
    if (rc != D3D_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(tx_number_kernel, dim3(ceil_div(m, TX_BLOCK)), dim3(TX_BLOCK), 0, st, key, label, m, number, chart);
        D3D_LAUNCH_CHECK("tx_number_kernel launch");
    }
    return D3D_OK;
}

extern "C" int d3d_texture_rects(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* key,
                                 const int* chart, long long n_charts, const d3d_ortho_view_t* cams, int n_cams, int pad, int* rect,
                                 d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && ((faces && key && chart) || n_faces == 0) && (rect || n_charts == 0),
                "null pointer (vertices, faces, key, chart, rect)");
    TX_CHECK_SIZES();
    TX_CHECK_VIEWS(cams, n_cams);
    D3D_REQUIRE(n_charts >= 0 && n_charts <= n_faces, "n_charts=%lld (0 .. n_faces)", n_charts);
    D3D_REQUIRE(pad >= 1 && pad < (1 << 20), "pad=%d (1 .. 2^20 - 1)", pad);
    if (n_charts == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tx_rect_init_kernel, dim3(ceil_div(4 * n_charts, TX_BLOCK)), dim3(TX_BLOCK), 0, st, rect, (long)n_charts);
    D3D_LAUNCH_CHECK("tx_rect_init_kernel launch");
    hipLaunchKernelGGL(tx_rects_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, st, vertices, n_vertices, faces, (long)n_faces,
                       key, chart, (long)n_charts, cams, n_cams, pad, rect);
    D3D_LAUNCH_CHECK("tx_rects_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_fill(const int* work, long long n_work, const int* table, long long n_charts, const long long* page_row,
                                int n_pages, const d3d_ortho_view_t* views, int n_views, int page_width, unsigned int* atlas,
                                d3d_stream_t stream) {
    D3D_REQUIRE((work || n_work == 0) && (table || n_charts == 0) && page_row && atlas, "null pointer (work, table, page_row, atlas)");
    D3D_REQUIRE(n_work >= 0 && n_work < (1ll << 31) / 4 && n_charts >= 0 && n_charts < (1ll << 31) && n_pages >= 1,
                "n_work=%lld, n_charts=%lld, n_pages=%d", n_work, n_charts, n_pages);
    D3D_REQUIRE(page_width >= 1, "page_width=%d", page_width);
    TX_CHECK_VIEWS(views, n_views);
    if (n_work == 0 || n_views == 0) return D3D_OK;
    hipLaunchKernelGGL(tx_fill_kernel, dim3(ceil_div(n_work, TX_BLOCK / 64)), dim3(TX_BLOCK), 0, (hipStream_t)stream, work, (long)n_work,
                       table, (long)n_charts, page_row, n_pages, views, n_views, page_width, atlas);
    D3D_LAUNCH_CHECK("tx_fill_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_empty(unsigned int* atlas, long long n_texels, unsigned int empty_rgba, d3d_stream_t stream) {
    D3D_REQUIRE(atlas || n_texels == 0, "null pointer (atlas)");
    D3D_REQUIRE(n_texels >= 0 && n_texels < (1ll << 40), "n_texels=%lld", n_texels);
    if (n_texels == 0) return D3D_OK;
    hipLaunchKernelGGL(tx_empty_kernel, dim3((unsigned)((n_texels + TX_BLOCK - 1) / TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream,
                       atlas, n_texels, empty_rgba | 0xff000000u);
    D3D_LAUNCH_CHECK("tx_empty_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_texcoords(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* key,
                                     const int* chart, const int* table, long long n_charts, const long long* page_row, int n_pages,
                                     const d3d_ortho_view_t* cams, int n_cams, int page_width, float* texcoord, int* texnumber,
                                     d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && ((faces && key && chart && texcoord && texnumber) || n_faces == 0) &&
                    (table || n_charts == 0) && page_row,
                "null pointer (vertices, faces, key, chart, table, page_row, texcoord, texnumber)");
    TX_CHECK_SIZES();
    TX_CHECK_VIEWS(cams, n_cams);
    D3D_REQUIRE(n_pages >= 1 && page_width >= 1 && n_charts >= 0, "n_pages=%d, page_width=%d, n_charts=%lld", n_pages, page_width, n_charts);
    if (n_faces == 0) return D3D_OK;
    hipLaunchKernelGGL(tx_texcoords_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream, vertices, n_vertices,
                       faces, (long)n_faces, key, chart, table, (long)n_charts, page_row, n_pages, cams, n_cams, page_width, texcoord,
                       texnumber);
    D3D_LAUNCH_CHECK("tx_texcoords_kernel launch");
    return D3D_OK;
}
