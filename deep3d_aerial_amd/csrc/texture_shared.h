// What the texture stage's files (texture.hip, texture_smooth.hip, texture_level.hip, texture_local.hip, texture_outliers.hip) share; not part of the public ABI.
#pragma once
#include <cmath>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int TX_BLOCK = 256;   // faces per select block (one workgroup), lanes per workgroup elsewhere
constexpr int TX_BAND = 8;      // atlas rows per fill work item
constexpr int TX_CANDIDATES = 16;   // keys per face of the candidate lists (d3d_texture_candidates_max)
constexpr long long TX_EMPTY = 0x7fffffffffffffffll;

struct TxFace {
    double a[3], b[3], c[3];
};

__device__ __forceinline__ bool tx_face(const float* __restrict__ vertices, const int* __restrict__ faces, long f, long long n, TxFace* F) {
    int ia, ib, ic;
    if (!geom_face<false>(faces, f, n, &ia, &ib, &ic)) return false;   // texture.py refuses them
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F->a[k] = (double)vertices[3l * ia + k];
        F->b[k] = (double)vertices[3l * ib + k];
        F->c[k] = (double)vertices[3l * ic + k];
    }
    return true;
}

// What the per-view tests need of a face: its corners, nrm = (b - a) x (c - a) and g = ((a + b) + c) / 3, in fp64.
struct TxFrame {
    TxFace F;
    double nrm[3], g[3];
};

// False for a face past m, with an index out of range or with nrm = 0: it gets no view.
__device__ __forceinline__ bool tx_frame(const float* __restrict__ vertices, const int* __restrict__ faces, long f, long m, long long n,
                                         TxFrame* T) {
    bool live = f < m && tx_face(vertices, faces, f, n, &T->F);
    const TxFace& F = T->F;
#pragma unroll
    for (int k = 0; k < 3; ++k) T->nrm[k] = T->g[k] = 0.0;
    if (live) {
        const double e1[3] = {F.b[0] - F.a[0], F.b[1] - F.a[1], F.b[2] - F.a[2]};
        const double e2[3] = {F.c[0] - F.a[0], F.c[1] - F.a[1], F.c[2] - F.a[2]};
        T->nrm[0] = e1[1] * e2[2] - e1[2] * e2[1];
        T->nrm[1] = e1[2] * e2[0] - e1[0] * e2[2];
        T->nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) T->g[k] = ((F.a[k] + F.b[k]) + F.c[k]) / 3.0;
        live = T->nrm[0] != 0.0 || T->nrm[1] != 0.0 || T->nrm[2] != 0.0;
    }
    return live;
}

// The tests of one view on one face (texture.py: Candidate, Choice): false when the view is no candidate, else *key =
// (bits(fp32(1 / A)) << 32) | id.  tol1 = 1 + depth_tolerance.  The selection and the candidate lists both call this.
__device__ __forceinline__ bool tx_view_key(const d3d_ortho_view_t& V, const TxFrame& T, double tol1, long long* key) {
    const TxFace& F = T.F;
    const double *nrm = T.nrm, *g = T.g;
    // front-facing: nrm . (C - g) > 0
    const double dot = nrm[0] * (V.C[0] - g[0]) + nrm[1] * (V.C[1] - g[1]) + nrm[2] * (V.C[2] - g[2]);
    if (!(dot > 0.0)) return false;
    double ua, va, ub, vb, uc, vc, p2;
    if (!geom_uv(V, F.a[0], F.a[1], F.a[2], &ua, &va, &p2)) return false;
    if (!geom_uv(V, F.b[0], F.b[1], F.b[2], &ub, &vb, &p2)) return false;
    if (!geom_uv(V, F.c[0], F.c[1], F.c[2], &uc, &vc, &p2)) return false;
    // the centroid has not been tested against the image, so ug + 0.5 is clamped before the floor: not geom_depth_at's rule
    const GeomPq r = geom_project(V, g[0], g[1], g[2]);
    const double ug = r.q0 / r.q2, vg = r.q1 / r.q2;
    const int px = min(max((int)floor(fmin(fmax(ug + 0.5, 0.0), (double)V.W)), 0), V.W - 1);
    const int py = min(max((int)floor(fmin(fmax(vg + 0.5, 0.0), (double)V.H)), 0), V.H - 1);
    const float D = V.depth[(long)py * V.W + px];
    if (!(isfinite(D) && D > 0.0f && r.p2 <= (double)D * tol1)) return false;
    const double A = 0.5 * fabs((ub - ua) * (vc - va) - (uc - ua) * (vb - va));
    if (!(A != 0.0)) return false;
    const double s = 1.0 / A;
    if (!isfinite(s)) return false;
    *key = geom_view_key(s, V.id);
    return true;
}

// The per-block cull of the selection (texture.hip): mask [ceil(m / TX_BLOCK), ceil(n_views / 64)] uint64, bit v of a block's
// words set when view v may see one of the block's faces.  tx_mask_bytes is the size of mask.
inline size_t tx_mask_bytes(long long m, int n_views) { return (size_t)ceil_div(m, TX_BLOCK) * ceil_div(n_views, 64) * 8; }
int tx_cull(const float* vertices, long long n, const int* faces, long long m, const d3d_ortho_view_t* views, int n_views,
            unsigned long long* mask, hipStream_t st);

// The view of `id` in a table sorted by id (lower bound), or -1.
__device__ __forceinline__ int tx_find(const d3d_ortho_view_t* __restrict__ views, int n_views, int id) {
    int lo = 0, hi = n_views;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (views[mid].id < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n_views && views[lo].id == id ? lo : -1;
}

// The (u, v) of face f's corners in view V: false when one is not in front or not finite (a key from another mesh or table).
__device__ __forceinline__ bool tx_corner_uv(const d3d_ortho_view_t& V, const TxFace& F, double* u, double* v) {
    const double* P[3] = {F.a, F.b, F.c};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const GeomPq r = geom_project(V, P[k][0], P[k][1], P[k][2]);
        if (!(r.p2 > 0.0 && r.q2 > 0.0)) return false;
        u[k] = r.q0 / r.q2;
        v[k] = r.q1 / r.q2;
        if (!(isfinite(u[k]) && isfinite(v[k]))) return false;
    }
    return true;
}

// A chart's row of the chart table [n_charts, 8] int32 (x0, y0, w, h, ox, oy, page, id) for the passes that work on the atlas
// (texture_level.hip, texture_local.hip).
struct TxlChart {
    int x0, y0, w, h, ox, oy;
    long long row0;   // the atlas row of the rect's first row
    int slot;         // of the chart's view in the camera table, -1: the chart is skipped
};

// The chart's rect, checked as the fill checks it: false for a bad row, which is then never read or written out of bounds.
__device__ __forceinline__ bool txl_rect(const int* __restrict__ table, long n_charts, int c, const long long* __restrict__ page_row,
                                         int n_pages, int P, TxlChart* C) {
    if (c < 0 || c >= n_charts) return false;
    const int* T = table + 8l * c;
    C->x0 = T[0], C->y0 = T[1], C->w = T[2], C->h = T[3], C->ox = T[4], C->oy = T[5];
    const int page = T[6];
    if (page < 0 || page >= n_pages) return false;
    C->row0 = page_row[page] + C->oy;
    return !(C->w < 1 || C->h < 1 || C->ox < 0 || C->ox + (long long)C->w > P || C->oy < 0 || C->row0 + C->h > page_row[page + 1]);
}

// The rect and the slot of the chart's view among the cameras (slot -1: a bad row or a missing view, the chart is skipped).
__device__ __forceinline__ TxlChart txl_chart(const int* __restrict__ table, long n_charts, int c, const long long* __restrict__ page_row,
                                              int n_pages, const d3d_ortho_view_t* __restrict__ cams, int n_cams, int P) {
    TxlChart C;
    C.slot = -1;
    if (txl_rect(table, n_charts, c, page_row, n_pages, P, &C)) C.slot = tx_find(cams, n_cams, table[8l * c + 7]);
    return C;
}

__device__ __forceinline__ double txl_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// The bilinear tap of the atlas at (x, y), atlas coordinates inside chart C, in fp64 and not rounded (texture.py "Sample"):
// pad >= 1 keeps the taps inside the rect; a rect clamped at the image's border repeats its last texel.
__device__ __forceinline__ void txl_tap(const TxlChart& C, int P, const unsigned* __restrict__ atlas, double x, double y, double* val) {
    const double xf = floor(x), yf = floor(y);
    const double tx = x - xf, ty = y - yf;
    const long long ix0 = (long long)txl_clamp(xf, (double)C.ox, (double)(C.ox + C.w - 1));
    const long long iy0 = (long long)txl_clamp(yf, (double)C.row0, (double)(C.row0 + C.h - 1));
    const long long ix1 = min(ix0 + 1, (long long)(C.ox + C.w - 1)), iy1 = min(iy0 + 1, C.row0 + C.h - 1);
    const unsigned c00 = atlas[iy0 * P + ix0], c10 = atlas[iy0 * P + ix1], c01 = atlas[iy1 * P + ix0], c11 = atlas[iy1 * P + ix1];
    const double w00 = (1.0 - tx) * (1.0 - ty), w10 = tx * (1.0 - ty), w01 = (1.0 - tx) * ty, w11 = tx * ty;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double a = (double)((c00 >> (8 * q)) & 255u), b = (double)((c10 >> (8 * q)) & 255u);
        const double c = (double)((c01 >> (8 * q)) & 255u), d = (double)((c11 >> (8 * q)) & 255u);
        val[q] = ((w00 * a + w10 * b) + w01 * c) + w11 * d;
    }
}

}  // namespace d3d
