// What the texture stage's two files (texture.hip, texture_level.hip) share; not part of the public ABI.
#pragma once
#include <cmath>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int TX_BLOCK = 256;   // faces per select block (one workgroup), lanes per workgroup elsewhere
constexpr int TX_BAND = 8;      // atlas rows per fill work item
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

}  // namespace d3d
