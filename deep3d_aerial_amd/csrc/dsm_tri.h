// The triangle coverage the mesh DSM (dsm.hip) and the orthophoto of the textured mesh (ortho_mesh.hip, §4.26)
// share: the raster, the set-up of a face, its cell range, the coverage test of a cell centre and the height sample.  One copy, so
// the two rasters cover the same cells with the same heights; not part of the public ABI.  Built with -ffp-contract=off.
//
// A triangle's vertices are put in lexicographic (x, y, z) order (IEEE total order per component: the order of the weighted sum
// then depends on the triangle alone, not on its winding or first vertex).  Edge p -> q has endpoints (u, v) in lexicographic
// (x, y) order and s = +1 if (u, v) == (p, q), else -1; E(p, q, P) = s ((v.x - u.x)(P.y - u.y) - (v.y - u.y)(P.x - u.x)), fp64,
// no contraction: two triangles sharing an edge evaluate the same magnitudes on it (watertight).  D = E(a, b, c); 0 or
// non-finite D: no contribution.  w_a = sigma E(b, c, P), w_b = sigma E(c, a, P), w_c = sigma E(a, b, P), sigma = sign(D);
// the centre is covered when all w >= 0 and W = (w_a + w_b) + w_c > 0, and the sample is
// fp32(((w_a z_a + w_b z_b) + w_c z_c) / W), dropped outside [z_min, z_max].
#pragma once
#include "geom_shared.h"

namespace d3d {

constexpr int DSM_BLOCK = 256;
constexpr int DSM_TRI_GRID = 1024;     // workgroups walking the list of larger triangles
constexpr int DSM_TRI_CHUNK = 256;     // cells of a listed triangle's range per chunk: one per lane

struct DsmGrid {
    double x_min, y_max, ux, uy, z_min, z_max;
    int W, H;
};

struct DsmTri {
    double ox[3], oy[3], ex[3], ey[3], t[3];   // edge k (opposite vertex k): origin u, direction v - u, s * sigma
    double z[3];
    double x_lo, x_hi, y_lo, y_hi;
};

__device__ __forceinline__ bool dsm_vtx_less(const float* p, const float* q) {
    const unsigned px = dsm_key(p[0]), qx = dsm_key(q[0]), py = dsm_key(p[1]), qy = dsm_key(q[1]);
    return px < qx || (px == qx && (py < qy || (py == qy && dsm_key(p[2]) < dsm_key(q[2]))));
}

// Swaps two vertices and the corners they came from.
__device__ __forceinline__ void dsm_vtx_swap(float* p, float* q, int* cp, int* cq) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = p[k];
        p[k] = q[k];
        q[k] = a;
    }
    const int c = *cp;
    *cp = *cq;
    *cq = c;
}

// Edge p -> q of the triangle (slot k): origin, direction and s.
__device__ __forceinline__ void dsm_edge(const float* p, const float* q, int k, DsmTri& T, double* s) {
    const bool fwd = p[0] < q[0] || (p[0] == q[0] && p[1] <= q[1]);
    const float* u = fwd ? p : q;
    const float* v = fwd ? q : p;
    T.ox[k] = (double)u[0];
    T.oy[k] = (double)u[1];
    T.ex[k] = (double)v[0] - (double)u[0];
    T.ey[k] = (double)v[1] - (double)u[1];
    *s = fwd ? 1.0 : -1.0;
}

__device__ __forceinline__ double dsm_edge_eval(const DsmTri& T, int k, double px, double py) {
    return T.ex[k] * (py - T.oy[k]) - T.ey[k] * (px - T.ox[k]);
}

// Face f -> its coverage data; false when the face contributes nothing (an index out of range, a non-finite coordinate, D 0
// or not finite).  corner[k] is the corner of the face (0, 1, 2) that became vertex k of the lexicographic order: what a caller
// with per-corner data (texcoords) sorts it by.  A face that passes has three distinct vertices, so the order is the face's alone.
__device__ __forceinline__ bool dsm_tri_setup(const float* __restrict__ vertices, int n_vertices, const int* __restrict__ faces, long f,
                                              DsmTri& T, int (&corner)[3]) {
    float v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        corner[c] = c;
        const int id = faces[3 * f + c];
        if (id < 0 || id >= n_vertices) return false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[c][a] = vertices[3 * (long)id + a];
            if (!isfinite(v[c][a])) return false;
        }
    }
    if (dsm_vtx_less(v[1], v[0])) dsm_vtx_swap(v[0], v[1], corner + 0, corner + 1);
    if (dsm_vtx_less(v[2], v[1])) dsm_vtx_swap(v[1], v[2], corner + 1, corner + 2);
    if (dsm_vtx_less(v[1], v[0])) dsm_vtx_swap(v[0], v[1], corner + 0, corner + 1);
    double s[3];
    dsm_edge(v[1], v[2], 0, T, s + 0);   // b -> c
    dsm_edge(v[2], v[0], 1, T, s + 1);   // c -> a
    dsm_edge(v[0], v[1], 2, T, s + 2);   // a -> b
    const double D = s[2] * dsm_edge_eval(T, 2, (double)v[2][0], (double)v[2][1]);
    if (!(D != 0.0 && isfinite(D))) return false;
    const double sigma = D > 0.0 ? 1.0 : -1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T.t[k] = s[k] * sigma;   // (s sigma) X == sigma (s X) exactly: both only set the sign
        T.z[k] = (double)v[k][2];
    }
    T.x_lo = (double)fminf(fminf(v[0][0], v[1][0]), v[2][0]);
    T.x_hi = (double)fmaxf(fmaxf(v[0][0], v[1][0]), v[2][0]);
    T.y_lo = (double)fminf(fminf(v[0][1], v[1][1]), v[2][1]);
    T.y_hi = (double)fmaxf(fmaxf(v[0][1], v[1][1]), v[2][1]);
    return true;
}

// The cell range (columns j0..j1, rows i0..i1) whose centres are tested; false when it misses the raster.
__device__ __forceinline__ bool dsm_tri_range(const DsmTri& T, const DsmGrid& g, int* j0, int* j1, int* i0, int* i1) {
    const double a = fmax(floor((T.x_lo - g.x_min) / g.ux) - 1.0, 0.0);
    const double b = fmin(floor((T.x_hi - g.x_min) / g.ux) + 1.0, (double)(g.W - 1));
    const double c = fmax(floor((g.y_max - T.y_hi) / g.uy) - 1.0, 0.0);
    const double d = fmin(floor((g.y_max - T.y_lo) / g.uy) + 1.0, (double)(g.H - 1));
    if (!(a <= b && c <= d)) return false;
    *j0 = (int)a;
    *j1 = (int)b;
    *i0 = (int)c;
    *i1 = (int)d;
    return true;
}

// The sample of the triangle at the centre of cell (i, j), if it covers it and the sample is inside the Z bounds; w and *W are
// the weights (w_a, w_b, w_c) and their sum, what a caller interpolates its own per-vertex data with.
__device__ __forceinline__ bool dsm_tri_sample(const DsmTri& T, const DsmGrid& g, int i, int j, float* z, double (&w)[3], double* W) {
    const double px = g.x_min + ((double)j + 0.5) * g.ux;
    const double py = g.y_max - ((double)i + 0.5) * g.uy;
    w[0] = T.t[0] * dsm_edge_eval(T, 0, px, py);
    w[1] = T.t[1] * dsm_edge_eval(T, 1, px, py);
    w[2] = T.t[2] * dsm_edge_eval(T, 2, px, py);
    if (!(w[0] >= 0.0 && w[1] >= 0.0 && w[2] >= 0.0)) return false;
    *W = (w[0] + w[1]) + w[2];
    if (!(*W > 0.0)) return false;
    const float s = (float)(((w[0] * T.z[0] + w[1] * T.z[1]) + w[2] * T.z[2]) / *W);
    const double sd = (double)s;
    if (!(sd >= g.z_min && sd <= g.z_max)) return false;
    *z = s;
    return true;
}

__device__ __forceinline__ bool dsm_tri_sample(const DsmTri& T, const DsmGrid& g, int i, int j, float* z) {
    double w[3], W;
    return dsm_tri_sample(T, g, i, j, z, w, &W);
}

// Chunk ownership of the persistent grid that walks a list of large triangles (dsm_tri_big_kernel states it): the first chunk of
// listed entry q that belongs to workgroup b of G, (q + k) mod G == b.
__device__ __forceinline__ int dsm_tri_first_chunk(int q, int b, int G) { return (b - q % G + G) % G; }

}  // namespace d3d
