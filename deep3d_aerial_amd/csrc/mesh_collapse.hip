// Collapsing the mesh edges shorter than the images resolve: the candidates of one round.  The rule is this
// project's (deep3d_aerial_amd/collapse.py states it in full, include/deep3d_planesweep.h too); it does not claim to match
// OpenMVS's RefineMesh.  The edge list is d3d_mesh_decimate_edges', the measure d3d_mesh_subdivide_measure's, and the winners are
// taken by the decimation's claim, apply and faces passes with every valid candidate eligible; this file adds the one pass
// between them.
//
// candidates: one lane per edge.  The tests run from cheap to dear, so a lane whose edge is not short does one load and two
//             stores: short (the measure), an end free (two bytes), the link condition (a merge of the two sorted neighbour
//             rows), the degree, the length guard (one walk of both rows, a position per neighbour), the flips (the two face
//             rows, three positions per face).  The validity tests are the decimation's own (geom_shared.h: dq_shared, dq_flips).
// No atomics; every float result is a fixed-order fp64 computation without contraction, so nothing depends on the order lanes
// run in.  No wave-wide operation follows the divergent exits.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int CL_BLOCK = 256;
constexpr unsigned CL_HASH = 2654435761u;

// The neighbours w of row v other than `other`: true when one of them would get an edge to t longer than the guard allows,
// |t - x_w|^2 s <= max2 failing (a NaN fails it).
__device__ __forceinline__ bool cl_too_long(const float* __restrict__ vertices, const long long* __restrict__ offset, const int* __restrict__ nbr,
                                            int v, int other, const double* t, double s, double max2) {
    const long long i1 = offset[v + 1];
    for (long long i = offset[v]; i < i1; ++i) {
        const int w = nbr[i];
        if (w == other) continue;
        double x[3];
        geom_load3(vertices, w, x);
        const double dx = t[0] - x[0], dy = t[1] - x[1], dz = t[2] - x[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 * s <= max2)) return true;
    }
    return false;
}

__global__ __launch_bounds__(CL_BLOCK) void cl_candidates_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                 const long long* __restrict__ offset, const int* __restrict__ nbr,
                                                                 const unsigned char* __restrict__ fixed, const int* __restrict__ foff,
                                                                 const int* __restrict__ finc, const int* __restrict__ edges,
                                                                 const long long* __restrict__ n_edges, long long max_edges,
                                                                 const double* __restrict__ measure, double min2, double max2,
                                                                 float* __restrict__ target, long long* __restrict__ key) {
    const long e = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (e >= max_edges) return;
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;
    long long k = -1;
    const double m = e < *n_edges ? measure[e] : 0.0;
    if (m > 0.0 && m < min2) {   // short, in a view that sees both ends
        const int a = edges[2 * e], b = edges[2 * e + 1];
        const bool fa = fixed[a] != 0, fb = fixed[b] != 0;
        // (1) the link condition: exactly two common neighbours; (2) the survivor keeps at least three neighbours
        bool valid = !(fa && fb) && dq_shared(offset, nbr, a, b) == 2 && (offset[a + 1] - offset[a]) + (offset[b + 1] - offset[b]) - 4 >= 3;
        if (valid) {
            double xa[3], xb[3], t[3];
            geom_load3(vertices, a, xa);
            geom_load3(vertices, b, xb);
            // a fixed end survives where it is; two free ends meet at the subdivision's midpoint
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = (double)(fa ? (float)xa[i] : (fb ? (float)xb[i] : (float)((xa[i] + xb[i]) * 0.5)));
            // (4) the guard: the survivor's edges, in the pixels per world unit of the collapsing edge
            const double dx = xb[0] - xa[0], dy = xb[1] - xa[1], dz = xb[2] - xa[2];
            const double s = m / ((dx * dx + dy * dy) + dz * dz);
            valid = !cl_too_long(vertices, offset, nbr, a, b, t, s, max2);
            if (valid) valid = !cl_too_long(vertices, offset, nbr, b, a, t, s, max2);
            // (3) no face turns over, judged at the fp32 position the survivor takes
            if (valid) valid = !dq_flips(vertices, faces, foff, finc, a, b, t);
            if (valid) valid = !dq_flips(vertices, faces, foff, finc, b, a, t);
            if (valid) {
                tx = (float)t[0], ty = (float)t[1], tz = (float)t[2];
                k = (long long)(((unsigned long long)__float_as_uint((float)m) << 32) | (unsigned long long)((unsigned)e * CL_HASH));
            }
        }
    }
    target[3 * e] = tx;
    target[3 * e + 1] = ty;
    target[3 * e + 2] = tz;
    key[e] = k;
}

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_mesh_collapse_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                            const long long* offset, const int* nbr, const unsigned char* fixed, const int* face_offset,
                                            const int* face_index, const int* edges, const long long* n_edges, long long max_edges,
                                            const double* measure, double min_edge, double max_edge, float* target, long long* key,
                                            d3d_stream_t stream) {
    D3D_REQUIRE(vertices && faces && offset && nbr && fixed && face_offset && face_index && edges && n_edges && measure && target && key,
                "null pointer (vertices, faces, offset, nbr, fixed, face_offset, face_index, edges, n_edges, measure, target, key)");
    D3D_REQUIRE(dq_sizes_ok(n_vertices, n_faces), "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 6 n_faces < 2^31)", n_vertices,
                n_faces);
    D3D_REQUIRE(max_edges >= 0 && max_edges < (1ll << 31), "max_edges=%lld (0 .. 2^31 - 1)", max_edges);
    D3D_REQUIRE(std::isfinite(min_edge) && min_edge > 0.0, "min_edge=%g must be a finite pixel length > 0", min_edge);
    D3D_REQUIRE(std::isfinite(max_edge) && max_edge >= 2.0 * min_edge, "max_edge=%g must be finite and >= 2 min_edge (%g)", max_edge,
                2.0 * min_edge);
    if (max_edges == 0) return D3D_OK;
    hipLaunchKernelGGL(cl_candidates_kernel, dim3(ceil_div(max_edges, CL_BLOCK)), dim3(CL_BLOCK), 0, (hipStream_t)stream, vertices, faces, offset,
                       nbr, fixed, face_offset, face_index, edges, n_edges, max_edges, measure, min_edge * min_edge, max_edge * max_edge, target,
                       key);
    D3D_LAUNCH_CHECK("cl_candidates_kernel launch");
    return D3D_OK;
}
