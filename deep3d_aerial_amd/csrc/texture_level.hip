// Levelling the colour seams between the texture's charts: the rules are this project's
// (deep3d_aerial_amd/texture.py states them, include/deep3d_planesweep.h too); they do not claim to match OpenMVS.
//
// graph:    per face the (chart, vertex) keys of its corners, every face's edges, per (edge, face) pair sorted by edge the seam
//           pairs of an edge with exactly two faces of different charts, per face its chart's smoothness edges; the caller
//           orders each list with torch.unique / torch.sort.  A CSR of the directed entries sorted by (row, column).
// samples:  one lane per node: a fp64 bilinear tap of the atlas; b per row of the CSR, its seam entries in column order.
// solve:    conjugate gradients on float4 node records.  An iteration is two streaming kernels, each followed by a one-workgroup
//           fold: matvec gathers r of the neighbours (one 16-byte load each) for s = A r and forms q = s + beta q, p = r + beta p
//           (A p = A r + beta A p_old), with per-workgroup fp64 partials of p . q; update does x += alpha p, r -= alpha q with
//           partials of r . r.  Partials go to fixed slots and are folded in slot order: no float atomics, the same bits on
//           every run.  alpha, beta, the norms and the per-channel done flags stay in device memory; the host reads the state
//           once per 16 iterations.
// coverage: one wave per face over its texel box grown by 2, clipped to the chart's rect: a 64-bit atomicMin of
//           (bits(fp32(d^2)) << 32) | face per texel with d^2 <= 2.
// apply:    one wave per (chart, band of rows), as the fill: coalesced 4-byte reads and writes.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"
#include "texture_shared.h"

namespace d3d {

constexpr int TXL_CHECK = 16;   // iterations between two reads of the solve's state by the host

// The index of key k in the sorted node keys, or -1.
__device__ __forceinline__ int txl_node(const long long* __restrict__ nodes, int n_nodes, long long k) {
    int lo = 0, hi = n_nodes;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nodes[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n_nodes && nodes[lo] == k ? lo : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// nodes and graph
// ---------------------------------------------------------------------------------------------------------------------------
// inc [3 m]: chart * n + vertex of each corner of a face with a chart, TX_EMPTY otherwise.
__global__ __launch_bounds__(TX_BLOCK) void txl_incidence_kernel(const int* __restrict__ faces, long m, long long n,
                                                                 const int* __restrict__ chart, long long* __restrict__ inc) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    long long e[3] = {TX_EMPTY, TX_EMPTY, TX_EMPTY};
    int a, b, c;
    const int ch = chart[f];
    if (geom_face<false>(faces, f, n, &a, &b, &c) && ch >= 0) {
        e[0] = (long long)ch * n + a;
        e[1] = (long long)ch * n + b;
        e[2] = (long long)ch * n + c;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) inc[3 * f + k] = e[k];
}

// face_node [3 m]: the node of each corner, -1 for a face with no chart.
__global__ __launch_bounds__(TX_BLOCK) void txl_face_nodes_kernel(const int* __restrict__ faces, long m, long long n,
                                                                  const int* __restrict__ chart, const long long* __restrict__ nodes,
                                                                  int n_nodes, int* __restrict__ face_node) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    int v[3], out[3] = {-1, -1, -1};
    const int ch = chart[f];
    if (geom_face<false>(faces, f, n, &v[0], &v[1], &v[2]) && ch >= 0)
        for (int k = 0; k < 3; ++k) out[k] = txl_node(nodes, n_nodes, (long long)ch * n + v[k]);
    if (out[0] < 0 || out[1] < 0 || out[2] < 0) out[0] = out[1] = out[2] = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) face_node[3 * f + k] = out[k];
}

// edge_key [3 m]: the distinct edges of EVERY face (with or without a winner) as min * n + max, TX_EMPTY in unused slots.
__global__ __launch_bounds__(TX_BLOCK) void txl_edges_kernel(const int* __restrict__ faces, long m, long long n,
                                                             long long* __restrict__ edge_key) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    long long e[3] = {TX_EMPTY, TX_EMPTY, TX_EMPTY};
    int a, b, c;
    if (geom_face<false>(faces, f, n, &a, &b, &c)) {
        int x[3], y[3];
        const int ne = geom_face_edges(a, b, c, x, y);
        for (int k = 0; k < ne; ++k) e[k] = (long long)min(x[k], y[k]) * n + max(x[k], y[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) edge_key[3 * f + k] = e[k];
}

// (edge, face) pairs sorted by edge.  The first pair of a run of exactly two whose faces lie in different charts emits the seam
// pairs of the edge's two ends: (node(c1, v) << 32) | node(c2, v), c1 < c2; every other slot gets TX_EMPTY.  seam [2 n_pairs].
__global__ __launch_bounds__(TX_BLOCK) void txl_seams_kernel(const long long* __restrict__ edge_sorted, const int* __restrict__ face_sorted,
                                                             long n_pairs, long m, long long n, const int* __restrict__ chart,
                                                             const long long* __restrict__ nodes, int n_nodes,
                                                             long long* __restrict__ seam) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= n_pairs) return;
    long long out[2] = {TX_EMPTY, TX_EMPTY};
    const long long e = edge_sorted[i];
    const bool first = i == 0 || edge_sorted[i - 1] != e;
    const bool two = i + 1 < n_pairs && edge_sorted[i + 1] == e && (i + 2 >= n_pairs || edge_sorted[i + 2] != e);
    if (e != TX_EMPTY && e >= 0 && first && two) {
        const int fa = face_sorted[i], fb = face_sorted[i + 1];
        if (fa >= 0 && fa < m && fb >= 0 && fb < m) {
            const int ca = chart[fa], cb = chart[fb];
            if (ca >= 0 && cb >= 0 && ca != cb) {
                const long long c1 = min(ca, cb), c2 = max(ca, cb);
                const long long v[2] = {e / n, e % n};
                for (int k = 0; k < 2; ++k) {
                    const int n1 = txl_node(nodes, n_nodes, c1 * n + v[k]), n2 = txl_node(nodes, n_nodes, c2 * n + v[k]);
                    if (n1 >= 0 && n2 >= 0) out[k] = ((long long)n1 << 32) | (long long)n2;
                }
            }
        }
    }
    seam[2 * i] = out[0];
    seam[2 * i + 1] = out[1];
}

// smooth [3 m]: the distinct edges of a face with a chart between its corners' nodes, (min << 32) | max.
__global__ __launch_bounds__(TX_BLOCK) void txl_smooth_kernel(const int* __restrict__ face_node, long m, long long* __restrict__ smooth) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    long long e[3] = {TX_EMPTY, TX_EMPTY, TX_EMPTY};
    const int a = face_node[3 * f], b = face_node[3 * f + 1], c = face_node[3 * f + 2];
    if (a >= 0 && b >= 0 && c >= 0) {
        int x[3], y[3];
        const int ne = geom_face_edges(a, b, c, x, y);
        for (int k = 0; k < ne; ++k) e[k] = ((long long)min(x[k], y[k]) << 32) | (long long)max(x[k], y[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) smooth[3 * f + k] = e[k];
}

// entry [nnz]: (row << 32) | column, sorted.  row_ptr [n_nodes + 1] (zeroed by the caller), column and weight [nnz]: 1 between
// nodes of different charts (a seam pair), lambda inside a chart.
__global__ __launch_bounds__(TX_BLOCK) void txl_csr_kernel(const long long* __restrict__ entry, long nnz, int n_nodes,
                                                           const long long* __restrict__ nodes, long long n, float lambda,
                                                           int* __restrict__ row_ptr, int* __restrict__ column, float* __restrict__ weight) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    const long long e = entry[i];
    const long long row = e >> 32, col = e & 0xffffffffll;
    const bool ok = row >= 0 && row < n_nodes && col < n_nodes;
    column[i] = ok ? (int)col : 0;
    weight[i] = ok ? (nodes[row] / n != nodes[col] / n ? 1.0f : lambda) : 0.0f;
    if (!ok) return;
    const long long prev = i > 0 ? min(max(entry[i - 1] >> 32, -1ll), row) : -1;
    for (long long r = prev + 1; r <= row; ++r) row_ptr[r] = (int)i;
    if (i == nnz - 1)
        for (long long r = row + 1; r <= n_nodes; ++r) row_ptr[r] = (int)nnz;
}

// ---------------------------------------------------------------------------------------------------------------------------
// samples and right-hand side
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TX_BLOCK) void txl_samples_kernel(const float* __restrict__ vertices, long long n,
                                                               const long long* __restrict__ nodes, int n_nodes,
                                                               const int* __restrict__ table, long n_charts,
                                                               const long long* __restrict__ page_row, int n_pages,
                                                               const d3d_ortho_view_t* __restrict__ cams, int n_cams, int P,
                                                               const unsigned* __restrict__ atlas, float4* __restrict__ f) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const long long k = nodes[i];
    const long long ch = k / n, v = k % n;
    const TxlChart C = txl_chart(table, n_charts, k >= 0 && ch < n_charts ? (int)ch : -1, page_row, n_pages, cams, n_cams, P);
    if (C.slot >= 0 && v >= 0) {
        const GeomPq r = geom_project(cams[C.slot], (double)vertices[3 * v], (double)vertices[3 * v + 1], (double)vertices[3 * v + 2]);
        const double u = r.q0 / r.q2, w = r.q1 / r.q2;
        if (r.p2 > 0.0 && r.q2 > 0.0 && isfinite(u) && isfinite(w)) {
            const double x = (u - (double)C.x0) + (double)C.ox;
            const double y = ((w - (double)C.y0) + (double)C.oy) + (double)(C.row0 - C.oy);
            double val[3];
            txl_tap(C, P, atlas, x, y, val);
            out = make_float4((float)val[0], (float)val[1], (float)val[2], 0.0f);
        }
    }
    f[i] = out;
}

// b[i] = the sum over row i's seam entries j (weight 1 between charts), in column order, of f[j] - f[i], in fp32.
__global__ __launch_bounds__(TX_BLOCK) void txl_rhs_kernel(const int* __restrict__ row_ptr, const int* __restrict__ column, long nnz,
                                                           const long long* __restrict__ nodes, long long n, int n_nodes,
                                                           const float4* __restrict__ f, float4* __restrict__ b) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    const float4 fi = f[i];
    const long long ci = nodes[i] / n;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const long e0 = max(row_ptr[i], 0), e1 = min((long)row_ptr[i + 1], nnz);
    for (long e = e0; e < e1; ++e) {
        const int j = column[e];
        if (j < 0 || j >= n_nodes || nodes[j] / n == ci) continue;
        const float4 fj = f[j];
        s.x += fj.x - fi.x;
        s.y += fj.y - fi.y;
        s.z += fj.z - fi.z;
    }
    b[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// conjugate gradients
// ---------------------------------------------------------------------------------------------------------------------------
struct TxlState {
    double rr[3], bb[3];
    float alpha[3], beta[3];
    int done[3];
    int all, iterations;
};

// The workgroup's sums of three fp64 values per lane to part[c * n_groups + blockIdx.x] (blockDim.x = TX_BLOCK).
__device__ __forceinline__ void txl_block_sums(double a, double b, double c, double* __restrict__ part, long n_groups) {
    __shared__ double lds[TX_BLOCK / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum(a), b = wave_sum(b), c = wave_sum(c);
    if (lane == 0) lds[wave][0] = a, lds[wave][1] = b, lds[wave][2] = c;
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = lds[0][threadIdx.x];
        for (int w = 1; w < TX_BLOCK / 64; ++w) s += lds[w][threadIdx.x];
        part[threadIdx.x * n_groups + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(TX_BLOCK) void txl_cg_init_kernel(const float4* __restrict__ b, int n_nodes, float4* __restrict__ x,
                                                               float4* __restrict__ r, float4* __restrict__ p, float4* __restrict__ q,
                                                               double* __restrict__ part, long n_groups) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    float4 bi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < n_nodes) {
        bi = b[i];
        bi.w = 0.0f;
        r[i] = bi;
        x[i] = p[i] = q[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    txl_block_sums((double)bi.x * (double)bi.x, (double)bi.y * (double)bi.y, (double)bi.z * (double)bi.z, part, n_groups);
}

// s = (L + mu I) r, one lane per row; q = s + beta q, p = r + beta p; partials of p . q.
__global__ __launch_bounds__(TX_BLOCK) void txl_cg_matvec_kernel(const int* __restrict__ row_ptr, const int* __restrict__ column,
                                                                 const float* __restrict__ weight, long nnz, int n_nodes, float mu,
                                                                 const float4* __restrict__ r, float4* __restrict__ p,
                                                                 float4* __restrict__ q, const TxlState* __restrict__ state,
                                                                 double* __restrict__ part, long n_groups) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (i < n_nodes) {
        const float b0 = state->beta[0], b1 = state->beta[1], b2 = state->beta[2];
        const float4 ri = r[i];
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, deg = 0.0f;
        const long e0 = max(row_ptr[i], 0), e1 = min((long)row_ptr[i + 1], nnz);
        for (long e = e0; e < e1; ++e) {
            const int j = column[e];
            if (j < 0 || j >= n_nodes) continue;
            const float w = weight[e];
            const float4 rj = r[j];
            a0 += w * rj.x;
            a1 += w * rj.y;
            a2 += w * rj.z;
            deg += w;
        }
        const float dm = deg + mu;
        const float4 qi = q[i], pi = p[i];
        float4 qn, pn;
        qn.x = (dm * ri.x - a0) + b0 * qi.x;
        qn.y = (dm * ri.y - a1) + b1 * qi.y;
        qn.z = (dm * ri.z - a2) + b2 * qi.z;
        qn.w = 0.0f;
        pn.x = ri.x + b0 * pi.x;
        pn.y = ri.y + b1 * pi.y;
        pn.z = ri.z + b2 * pi.z;
        pn.w = 0.0f;
        q[i] = qn;
        p[i] = pn;
        d0 = (double)pn.x * (double)qn.x, d1 = (double)pn.y * (double)qn.y, d2 = (double)pn.z * (double)qn.z;
    }
    txl_block_sums(d0, d1, d2, part, n_groups);
}

// x += alpha p, r -= alpha q; partials of r . r.
__global__ __launch_bounds__(TX_BLOCK) void txl_cg_update_kernel(int n_nodes, const float4* __restrict__ p, const float4* __restrict__ q,
                                                                 float4* __restrict__ x, float4* __restrict__ r,
                                                                 const TxlState* __restrict__ state, double* __restrict__ part, long n_groups) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (i < n_nodes) {
        const float a0 = state->alpha[0], a1 = state->alpha[1], a2 = state->alpha[2];
        const float4 pi = p[i], qi = q[i];
        float4 xi = x[i], ri = r[i];
        xi.x += a0 * pi.x, xi.y += a1 * pi.y, xi.z += a2 * pi.z;
        ri.x -= a0 * qi.x, ri.y -= a1 * qi.y, ri.z -= a2 * qi.z;
        x[i] = xi;
        r[i] = ri;
        d0 = (double)ri.x * (double)ri.x, d1 = (double)ri.y * (double)ri.y, d2 = (double)ri.z * (double)ri.z;
    }
    txl_block_sums(d0, d1, d2, part, n_groups);
}

// One workgroup folds the partials in slot order and steps the state.  mode 0: r = b (bb = rr, beta = 0); 1: the sums are p . q
// (alpha = rr / pq); 2: the sums are the new r . r (beta = new / old, the done flags, the iteration count).
__global__ __launch_bounds__(TX_BLOCK) void txl_cg_fold_kernel(const double* __restrict__ part, long n_groups, int mode, double tol2,
                                                               TxlState* __restrict__ state) {
    __shared__ double lds[TX_BLOCK / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c)
        for (long k = threadIdx.x; k < n_groups; k += TX_BLOCK) s[c] += part[c * n_groups + k];
    for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
    if (lane == 0)
        for (int c = 0; c < 3; ++c) lds[wave][c] = s[c];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const bool was_all = mode != 0 && state->all != 0;
    for (int c = 0; c < 3; ++c) {
        double t = lds[0][c];
        for (int w = 1; w < TX_BLOCK / 64; ++w) t += lds[w][c];
        if (mode == 0) {
            state->rr[c] = state->bb[c] = t;
            state->alpha[c] = state->beta[c] = 0.0f;
            state->done[c] = t <= tol2 * t ? 1 : 0;
        } else if (mode == 1) {
            state->alpha[c] = state->done[c] || !(t > 0.0) ? 0.0f : (float)(state->rr[c] / t);
        } else if (!state->done[c]) {
            state->beta[c] = (float)(t / state->rr[c]);
            state->rr[c] = t;
            if (t <= tol2 * state->bb[c]) state->done[c] = 1, state->beta[c] = 0.0f;
        } else {
            state->beta[c] = 0.0f;
        }
    }
    if (mode == 0) state->iterations = 0;
    if (mode == 2 && !was_all) state->iterations += 1;
    if (mode != 1) state->all = state->done[0] && state->done[1] && state->done[2] ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// coverage and apply
// ---------------------------------------------------------------------------------------------------------------------------
// The closest point of the triangle (X, Y)[0..2] to (px, py) in fp64: its barycentric weights w and the squared distance, 0
// inside (Ericson's regions: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, inside, tested in that order).
__device__ __forceinline__ double txl_closest(const double* X, const double* Y, double px, double py, double* w) {
    const double abx = X[1] - X[0], aby = Y[1] - Y[0], acx = X[2] - X[0], acy = Y[2] - Y[0];
    const double apx = px - X[0], apy = py - Y[0];
    const double d1 = abx * apx + aby * apy, d2 = acx * apx + acy * apy;
    const double bpx = px - X[1], bpy = py - Y[1];
    const double d3 = abx * bpx + aby * bpy, d4 = acx * bpx + acy * bpy;
    const double cpx = px - X[2], cpy = py - Y[2];
    const double d5 = abx * cpx + aby * cpy, d6 = acx * cpx + acy * cpy;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {
        w[0] = 1.0, w[1] = 0.0, w[2] = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {
        w[0] = 0.0, w[1] = 1.0, w[2] = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        w[0] = 1.0 - v, w[1] = v, w[2] = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {
        w[0] = 0.0, w[1] = 0.0, w[2] = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double t = d2 / (d2 - d6);
        w[0] = 1.0 - t, w[1] = 0.0, w[2] = t;
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        w[0] = 0.0, w[1] = 1.0 - t, w[2] = t;
    } else {
        const double den = 1.0 / ((va + vb) + vc);
        const double v = vb * den, t = vc * den;
        w[0] = (1.0 - v) - t, w[1] = v, w[2] = t;
        return isfinite(w[0]) && isfinite(v) && isfinite(t) ? 0.0 : INFINITY;
    }
    const double qx = (w[0] * X[0] + w[1] * X[1]) + w[2] * X[2], qy = (w[0] * Y[0] + w[1] * Y[1]) + w[2] * Y[2];
    const double dx = px - qx, dy = py - qy;
    return dx * dx + dy * dy;   // NaN (a degenerate triangle) is no candidate
}

// The corners of face f in texel coordinates of its chart's page: X = (u - x0) + ox, Y = (v - y0) + oy.
__device__ __forceinline__ bool txl_face_texels(const float* __restrict__ vertices, const int* __restrict__ faces, long f, long long n,
                                                const d3d_ortho_view_t& V, const TxlChart& C, double* X, double* Y) {
    TxFace F;
    double u[3], v[3];
    if (!(tx_face(vertices, faces, f, n, &F) && tx_corner_uv(V, F, u, v))) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        X[k] = (u[k] - (double)C.x0) + (double)C.ox;
        Y[k] = (v[k] - (double)C.y0) + (double)C.oy;
    }
    return true;
}

// One wave per face.  cover [atlas rows, P] int64, TX_EMPTY before.
__global__ __launch_bounds__(TX_BLOCK) void txl_cover_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                             long m, const int* __restrict__ chart, const int* __restrict__ table,
                                                             long n_charts, const long long* __restrict__ page_row, int n_pages,
                                                             const d3d_ortho_view_t* __restrict__ cams, int n_cams, int P,
                                                             long long* __restrict__ cover) {
    const long f = ((long)blockIdx.x * TX_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (f >= m) return;   // whole waves
    const TxlChart C = txl_chart(table, n_charts, chart[f], page_row, n_pages, cams, n_cams, P);
    if (C.slot < 0) return;
    double X[3], Y[3];
    if (!txl_face_texels(vertices, faces, f, n, cams[C.slot], C, X, Y)) return;
    const double xlo = (double)C.ox, xhi = (double)(C.ox + C.w - 1), ylo = (double)C.oy, yhi = (double)(C.oy + C.h - 1);
    const double bx0 = floor(fmin(fmin(X[0], X[1]), X[2])) - 2.0, bx1 = ceil(fmax(fmax(X[0], X[1]), X[2])) + 2.0;
    const double by0 = floor(fmin(fmin(Y[0], Y[1]), Y[2])) - 2.0, by1 = ceil(fmax(fmax(Y[0], Y[1]), Y[2])) + 2.0;
    if (bx1 < xlo || bx0 > xhi || by1 < ylo || by0 > yhi) return;
    const int ix0 = (int)txl_clamp(bx0, xlo, xhi), ix1 = (int)txl_clamp(bx1, xlo, xhi);
    const int iy0 = (int)txl_clamp(by0, ylo, yhi), iy1 = (int)txl_clamp(by1, ylo, yhi);
    const long bw = ix1 - ix0 + 1, total = bw * (iy1 - iy0 + 1);
    const long long row_of_page = C.row0 - C.oy;
    for (long i = lane; i < total; i += 64) {
        const int ty = iy0 + (int)(i / bw), tx = ix0 + (int)(i - (i / bw) * bw);
        double w[3];
        const double d2 = txl_closest(X, Y, (double)tx, (double)ty, w);
        if (!(d2 <= 2.0)) continue;
        const long long k = ((long long)__float_as_uint((float)d2) << 32) | (long long)f;
        atomicMin(cover + (row_of_page + ty) * (long long)P + tx, k);
    }
}

// One wave per (chart, band of rows).  g [n_nodes] float4.
__global__ __launch_bounds__(TX_BLOCK) void txl_apply_kernel(const int* __restrict__ work, long n_work, const float* __restrict__ vertices,
                                                             long long n, const int* __restrict__ faces, long m,
                                                             const int* __restrict__ chart, const int* __restrict__ face_node,
                                                             const float4* __restrict__ g, int n_nodes, const int* __restrict__ table,
                                                             long n_charts, const long long* __restrict__ page_row, int n_pages,
                                                             const d3d_ortho_view_t* __restrict__ cams, int n_cams, int P,
                                                             const long long* __restrict__ cover, unsigned* __restrict__ atlas) {
    const long item = ((long)blockIdx.x * TX_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (item >= n_work) return;   // whole waves
    const int c = work[2 * item], band = work[2 * item + 1];
    const TxlChart C = txl_chart(table, n_charts, c, page_row, n_pages, cams, n_cams, P);
    if (C.slot < 0 || band < 0) return;
    const long r_begin = (long)band * TX_BAND;
    const long rows = min((long)TX_BAND, C.h - r_begin);
    if (rows <= 0) return;
    const long total = rows * C.w;
    for (long i = lane; i < total; i += 64) {
        const int dy = (int)(r_begin + i / C.w), dx = (int)(i - (i / C.w) * C.w);
        const long long at = (C.row0 + dy) * (long long)P + C.ox + dx;
        const long long k = cover[at];
        if (k == TX_EMPTY) continue;
        const long f = (long)(k & 0xffffffffll);
        if (f >= m || chart[f] != c) continue;
        const int n0 = face_node[3 * f], n1 = face_node[3 * f + 1], n2 = face_node[3 * f + 2];
        if (n0 < 0 || n0 >= n_nodes || n1 < 0 || n1 >= n_nodes || n2 < 0 || n2 >= n_nodes) continue;
        double X[3], Y[3], w[3];
        if (!txl_face_texels(vertices, faces, f, n, cams[C.slot], C, X, Y)) continue;
        txl_closest(X, Y, (double)(C.ox + dx), (double)(C.oy + dy), w);
        const float w0 = (float)w[0], w1 = (float)w[1], w2 = (float)w[2];
        const float4 g0 = g[n0], g1 = g[n1], g2 = g[n2];
        const float cr[3] = {(w0 * g0.x + w1 * g1.x) + w2 * g2.x, (w0 * g0.y + w1 * g1.y) + w2 * g2.y, (w0 * g0.z + w1 * g1.z) + w2 * g2.z};
        const unsigned t = atlas[at];
        unsigned out = t & 0xff000000u;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float val = fminf(fmaxf(rintf((float)((t >> (8 * q)) & 255u) + cr[q]), 0.0f), 255.0f);
            out |= (val == val ? (unsigned)val : (t >> (8 * q)) & 255u) << (8 * q);   // a NaN correction keeps the colour
        }
        atlas[at] = out;
    }
}

struct TxlScratch {
    size_t r, p, q, part, state, bytes;
};

static TxlScratch txl_layout(long long n_nodes) {
    const size_t nn = (size_t)(n_nodes > 0 ? n_nodes : 1);
    ScratchLayout L;
    TxlScratch s;
    s.r = L.take(nn * 16);
    s.p = L.take(nn * 16);
    s.q = L.take(nn * 16);
    s.part = L.take((size_t)ceil_div((long)nn, TX_BLOCK) * 3 * 8);
    s.state = L.take(sizeof(TxlState));
    s.bytes = L.bytes;
    return s;
}

static bool txl_sizes_ok(long long n, long long m) { return n >= 0 && n < (1ll << 31) && m >= 0 && 3 * m < (1ll << 31); }

}  // namespace d3d

using namespace d3d;

#define TXL_CHECK_SIZES()                                                                                                           \
    D3D_REQUIRE(txl_sizes_ok(n_vertices, n_faces), "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 3 n_faces < 2^31)", n_vertices, \
                n_faces)

#define TXL_CHECK_NODES()                                                                                            \
    D3D_REQUIRE(n_nodes >= 0 && n_nodes < (1ll << 31), "n_nodes=%lld (0 .. 2^31 - 1)", n_nodes);                    \
    D3D_REQUIRE(nodes || n_nodes == 0, "null pointer (nodes)")

#define TXL_CHECK_TABLE()                                                                                                         \
    D3D_REQUIRE((table || n_charts == 0) && page_row && n_pages >= 1 && page_width >= 1 && n_charts >= 0 && n_charts < (1ll << 31), \
                "table, page_row, n_pages=%d, page_width=%d, n_charts=%lld", n_pages, page_width, n_charts);                      \
    D3D_REQUIRE(n_cams >= 0 && n_cams < (1 << 20) && (cams || n_cams == 0), "%d cameras (0 .. 2^20 - 1)", n_cams)

#define TXL_LAUNCH(kernel, count, ...)                                                                              \
    do {                                                                                                            \
        if ((count) > 0) {                                                                                          \
            hipLaunchKernelGGL(kernel, dim3(ceil_div((count), TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); \
            D3D_LAUNCH_CHECK(#kernel " launch");                                                                    \
        }                                                                                                           \
    } while (0)

extern "C" size_t d3d_texture_level_scratch_bytes(long long n_nodes) {
    if (n_nodes < 0 || n_nodes >= (1ll << 31)) return 0;
    return txl_layout(n_nodes).bytes;
}

extern "C" int d3d_texture_level_incidence(const int* faces, long long n_faces, long long n_vertices, const int* chart,
                                           long long* incidence, long long* edge_key, d3d_stream_t stream) {
    D3D_REQUIRE((faces && chart && incidence && edge_key) || n_faces == 0, "null pointer (faces, chart, incidence, edge_key)");
    TXL_CHECK_SIZES();
    TXL_LAUNCH(txl_incidence_kernel, (long)n_faces, faces, (long)n_faces, n_vertices, chart, incidence);
    TXL_LAUNCH(txl_edges_kernel, (long)n_faces, faces, (long)n_faces, n_vertices, edge_key);
    return D3D_OK;
}

extern "C" int d3d_texture_level_pairs(const int* faces, long long n_faces, long long n_vertices, const int* chart,
                                       const long long* nodes, long long n_nodes, const long long* edge_sorted, const int* face_sorted,
                                       long long n_pairs, int* face_node, long long* seam, long long* smooth, d3d_stream_t stream) {
    D3D_REQUIRE((faces && chart && face_node && smooth) || n_faces == 0, "null pointer (faces, chart, face_node, smooth)");
    D3D_REQUIRE((edge_sorted && face_sorted && seam) || n_pairs == 0, "null pointer (edge_sorted, face_sorted, seam)");
    TXL_CHECK_SIZES();
    TXL_CHECK_NODES();
    D3D_REQUIRE(n_pairs >= 0 && n_pairs <= 3 * n_faces, "n_pairs=%lld (0 .. 3 n_faces)", n_pairs);
    TXL_LAUNCH(txl_face_nodes_kernel, (long)n_faces, faces, (long)n_faces, n_vertices, chart, nodes, (int)n_nodes, face_node);
    TXL_LAUNCH(txl_seams_kernel, (long)n_pairs, edge_sorted, face_sorted, (long)n_pairs, (long)n_faces, n_vertices, chart, nodes,
               (int)n_nodes, seam);
    TXL_LAUNCH(txl_smooth_kernel, (long)n_faces, face_node, (long)n_faces, smooth);
    return D3D_OK;
}

extern "C" int d3d_texture_level_csr(const long long* entry, long long n_entries, const long long* nodes, long long n_nodes,
                                     long long n_vertices, float smooth, int* row_ptr, int* column, float* weight, d3d_stream_t stream) {
    D3D_REQUIRE(row_ptr && ((entry && column && weight) || n_entries == 0), "null pointer (entry, row_ptr, column, weight)");
    TXL_CHECK_NODES();
    D3D_REQUIRE(n_entries >= 0 && n_entries < (1ll << 31) && n_vertices >= 1 && n_vertices < (1ll << 31), "n_entries=%lld, n_vertices=%lld",
                n_entries, n_vertices);
    D3D_REQUIRE(std::isfinite(smooth) && smooth >= 0.0f, "smooth=%g must be finite and >= 0", (double)smooth);
    int rc = hip_status(hipMemsetAsync(row_ptr, 0, (size_t)(n_nodes + 1) * 4, (hipStream_t)stream), "texture level csr: clear row_ptr");
    if (rc != D3D_OK) return rc;
    TXL_LAUNCH(txl_csr_kernel, (long)n_entries, entry, (long)n_entries, (int)n_nodes, nodes, n_vertices, smooth, row_ptr, column, weight);
    return D3D_OK;
}

extern "C" int d3d_texture_level_samples(const float* vertices, long long n_vertices, const long long* nodes, long long n_nodes,
                                         const int* row_ptr, const int* column, long long n_entries, const int* table, long long n_charts,
                                         const long long* page_row, int n_pages, const d3d_ortho_view_t* cams, int n_cams, int page_width,
                                         const unsigned int* atlas, float* f, float* b, d3d_stream_t stream) {
    D3D_REQUIRE(((vertices && row_ptr && f && b && atlas) || n_nodes == 0) && (column || n_entries == 0),
                "null pointer (vertices, row_ptr, column, atlas, f, b)");
    TXL_CHECK_NODES();
    TXL_CHECK_TABLE();
    D3D_REQUIRE(n_vertices >= 1 && n_vertices < (1ll << 31) && n_entries >= 0 && n_entries < (1ll << 31), "n_vertices=%lld, n_entries=%lld",
                n_vertices, n_entries);
    TXL_LAUNCH(txl_samples_kernel, (long)n_nodes, vertices, n_vertices, nodes, (int)n_nodes, table, (long)n_charts, page_row, n_pages, cams,
               n_cams, page_width, atlas, (float4*)f);
    TXL_LAUNCH(txl_rhs_kernel, (long)n_nodes, row_ptr, column, (long)n_entries, nodes, n_vertices, (int)n_nodes, (const float4*)f,
               (float4*)b);
    return D3D_OK;
}

extern "C" int d3d_texture_level_solve(const int* row_ptr, const int* column, const float* weight, long long n_entries, const float* b,
                                       long long n_nodes, float anchor, double tolerance, int max_iterations, void* scratch,
                                       size_t scratch_bytes, float* g, int* iterations, int* converged, d3d_stream_t stream) {
    D3D_REQUIRE(((row_ptr && b && g) || n_nodes == 0) && ((column && weight) || n_entries == 0) && scratch && iterations && converged,
                "null pointer (row_ptr, column, weight, b, g, scratch, iterations, converged)");
    D3D_REQUIRE(n_nodes >= 0 && n_nodes < (1ll << 31) && n_entries >= 0 && n_entries < (1ll << 31), "n_nodes=%lld, n_entries=%lld", n_nodes,
                n_entries);
    D3D_REQUIRE(std::isfinite(anchor) && anchor > 0.0f, "anchor=%g must be finite and > 0", (double)anchor);
    D3D_REQUIRE(tolerance > 0.0 && tolerance < 1.0, "tolerance=%g must lie in (0, 1)", tolerance);
    D3D_REQUIRE(max_iterations >= 1, "max_iterations=%d must be >= 1", max_iterations);
    const TxlScratch L = txl_layout(n_nodes);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed (d3d_texture_level_scratch_bytes)", scratch_bytes, L.bytes);
    *iterations = 0;
    *converged = 1;
    if (n_nodes == 0) return D3D_OK;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    float4 *x = (float4*)g, *r = (float4*)(w + L.r), *p = (float4*)(w + L.p), *q = (float4*)(w + L.q);
    double* part = (double*)(w + L.part);
    TxlState* state = (TxlState*)(w + L.state);
    const long N = (long)n_nodes, groups = ceil_div(N, TX_BLOCK);
    const double tol2 = tolerance * tolerance;
    TxlState host;
    TXL_LAUNCH(txl_cg_init_kernel, N, (const float4*)b, (int)N, x, r, p, q, part, groups);
    hipLaunchKernelGGL(txl_cg_fold_kernel, dim3(1), dim3(TX_BLOCK), 0, st, part, groups, 0, tol2, state);
    D3D_LAUNCH_CHECK("txl_cg_fold_kernel launch");
    int launched = 0;
    for (;;) {
        int rc = hip_status(hipMemcpyAsync(&host, state, sizeof(TxlState), hipMemcpyDeviceToHost, st), "texture level solve: read state");
        if (rc != D3D_OK) return rc;
        rc = hip_status(hipStreamSynchronize(st), "texture level solve: sync");
        if (rc != D3D_OK) return rc;
        if (host.all || launched >= max_iterations) break;
        const int chunk = max_iterations - launched < TXL_CHECK ? max_iterations - launched : TXL_CHECK;
        for (int k = 0; k < chunk; ++k) {
            TXL_LAUNCH(txl_cg_matvec_kernel, N, row_ptr, column, weight, (long)n_entries, (int)N, anchor, r, p, q, state, part, groups);
            hipLaunchKernelGGL(txl_cg_fold_kernel, dim3(1), dim3(TX_BLOCK), 0, st, part, groups, 1, tol2, state);
            D3D_LAUNCH_CHECK("txl_cg_fold_kernel launch");
            TXL_LAUNCH(txl_cg_update_kernel, N, (int)N, p, q, x, r, state, part, groups);
            hipLaunchKernelGGL(txl_cg_fold_kernel, dim3(1), dim3(TX_BLOCK), 0, st, part, groups, 2, tol2, state);
            D3D_LAUNCH_CHECK("txl_cg_fold_kernel launch");
        }
        launched += chunk;
    }
    *iterations = host.iterations;
    *converged = host.all;
    return D3D_OK;
}

extern "C" int d3d_texture_level_cover(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* chart,
                                       const int* table, long long n_charts, const long long* page_row, int n_pages,
                                       const d3d_ortho_view_t* cams, int n_cams, int page_width, long long* cover, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && ((faces && chart && cover) || n_faces == 0), "null pointer (vertices, faces, chart, cover)");
    TXL_CHECK_SIZES();
    TXL_CHECK_TABLE();
    TXL_LAUNCH(txl_cover_kernel, (long)n_faces * 64, vertices, n_vertices, faces, (long)n_faces, chart, table, (long)n_charts, page_row,
               n_pages, cams, n_cams, page_width, cover);
    return D3D_OK;
}

extern "C" int d3d_texture_level_apply(const int* work, long long n_work, const float* vertices, long long n_vertices, const int* faces,
                                       long long n_faces, const int* chart, const int* face_node, const float* g, long long n_nodes,
                                       const int* table, long long n_charts, const long long* page_row, int n_pages,
                                       const d3d_ortho_view_t* cams, int n_cams, int page_width, const long long* cover,
                                       unsigned int* atlas, d3d_stream_t stream) {
    D3D_REQUIRE((work || n_work == 0) && (vertices || n_vertices == 0) && ((faces && chart && face_node) || n_faces == 0) &&
                    (g || n_nodes == 0) && cover && atlas,
                "null pointer (work, vertices, faces, chart, face_node, g, cover, atlas)");
    TXL_CHECK_SIZES();
    TXL_CHECK_TABLE();
    D3D_REQUIRE(n_work >= 0 && n_work < (1ll << 31) / 64 && n_nodes >= 0 && n_nodes < (1ll << 31), "n_work=%lld, n_nodes=%lld", n_work,
                n_nodes);
    TXL_LAUNCH(txl_apply_kernel, (long)n_work * 64, work, (long)n_work, vertices, n_vertices, faces, (long)n_faces, chart, face_node,
               (const float4*)g, (int)n_nodes, table, (long)n_charts, page_row, n_pages, cams, n_cams, page_width, cover, atlas);
    return D3D_OK;
}
