// Flipping the mesh edges whose flip removes a cap triangle: the candidates, the claim and the apply pass of
// one round.  The rule is this project's (deep3d_aerial_amd/flip.py states it in full, include/deep3d_planesweep.h too);
// it does not claim to match OpenMVS's bRemoveSpikes (VCG's RemoveTVertexByFlip).  The adjacency is d3d_mesh_adjacency's, the
// incidence d3d_mesh_decimate_incidence's and the edge list d3d_mesh_decimate_edges'.
//
// candidates: one lane per edge (a, b), a < b.  The tests run from cheap to dear, so a lane on a boundary edge does one short
//             row walk and two stores: the pair (a's face row: exactly two faces hold b, one a->b with the corner c opposite, one
//             b->a with d), c != d, the degrees (four offsets), the new edge (c's sorted neighbour row must not hold d), then
//             four positions: the planarity guard, no face turning over, the gain of the worse quality.
// claim:      claim[v] = the largest int64, then every candidate takes the 64-bit minimum of the keys on a, b, c and d.
// apply:      the faces are copied, then one lane per edge; a candidate that reads its own key back on all four is a winner and writes its two face slots.
//             Winners share no vertex, hence no face: plain stores.  A lane takes 32 edges and no lane leaves early, so the
//             winners are counted by one sum and one add per wave.
// Integer atomics only (the claim's atomicMin, the winners' counter); every float result is a fixed-order fp64 computation
// without contraction, so nothing depends on the order lanes run in.  In the candidates no wave-wide operation follows the
// divergent exits.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int FL_BLOCK = 256;
constexpr unsigned FL_HASH = 2654435761u;

__device__ __forceinline__ double fl_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ double fl_d2(const double* p, const double* q) {
    const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// Q = |n|^2 / S^2 of the triangle whose corners p0, p1, p2 come in increasing index order: n = (p1 - p0) x (p2 - p0),
// S = (|p1 - p0|^2 + |p2 - p1|^2) + |p0 - p2|^2; 0 when S is 0.
__device__ __forceinline__ double fl_quality_sorted(const double* p0, const double* p1, const double* p2) {
    double nrm[3];
    dq_normal(p0, p1, p2, nrm);
    const double s = (fl_d2(p0, p1) + fl_d2(p1, p2)) + fl_d2(p2, p0);
    return s == 0.0 ? 0.0 : fl_dot(nrm, nrm) / (s * s);
}

// Q of the triangle with the indices i, j, k at the positions x, y, z: a function of the vertex set, whatever the order given.
// The three exchanges of the sort are selects on the values, not on pointers, so the positions stay in registers.
__device__ __forceinline__ double fl_quality(int i, const double* x, int j, const double* y, int k, const double* z) {
    double p0[3], p1[3], p2[3];
    const bool s01 = i > j;
    const int lo = s01 ? j : i, mid = s01 ? i : j;
    const bool s12 = mid > k, s02 = lo > (s12 ? k : mid);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double u = s01 ? y[c] : x[c], v = s01 ? x[c] : y[c];   // (u, v) go with (lo, mid)
        const double w = s12 ? z[c] : v;                             // w goes with min(mid, k)
        p2[c] = s12 ? v : z[c];
        p0[c] = s02 ? w : u;
        p1[c] = s02 ? u : w;
    }
    return fl_quality_sorted(p0, p1, p2);
}

// The smaller of two qualities; y when the comparison fails (a NaN).
__device__ __forceinline__ double fl_min(double x, double y) { return x < y ? x : y; }

__global__ __launch_bounds__(FL_BLOCK) void fl_candidates_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                 const long long* __restrict__ offset, const int* __restrict__ nbr,
                                                                 const int* __restrict__ foff, const int* __restrict__ finc,
                                                                 const int* __restrict__ edges, const long long* __restrict__ n_edges,
                                                                 long long max_edges, double cos2, long long* __restrict__ key,
                                                                 int* __restrict__ opp) {
    const long e = (long)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (e >= max_edges) return;
    long long k = -1;
    int c = 0, d = 0, f_ab = 0, f_ba = 0;
    if (e < *n_edges) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        // (3) the pair: exactly two faces of a's row hold b, one as a->b and one as b->a
        int held = 0, n_ab = 0;
        const int o1 = foff[a + 1];
        for (int o = foff[a]; o < o1; ++o) {
            const int f = finc[o];
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            if (i0 != b && i1 != b && i2 != b) continue;
            ++held;
            // the corner after a in the face's cyclic order is b (a->b), or it is the opposite corner (b->a)
            const int next = i0 == a ? i1 : (i1 == a ? i2 : i0), prev = i0 == a ? i2 : (i1 == a ? i0 : i1);
            if (next == b) {
                ++n_ab;
                c = prev, f_ab = f;
            } else {
                d = next, f_ba = f;
            }
        }
        bool valid = held == 2 && n_ab == 1 && c != d;
        // (4.2) each end loses a neighbour
        if (valid) valid = offset[a + 1] - offset[a] > 3 && offset[b + 1] - offset[b] > 3;
        // (4.1) the new edge c-d must not exist yet
        if (valid) {
            const long long i1 = offset[c + 1];
            for (long long i = offset[c]; valid && i < i1; ++i) valid = nbr[i] != d;
        }
        if (valid) {
            double xa[3], xb[3], xc[3], xd[3], n1[3], n2[3], m1[3], m2[3], sum[3];
            geom_load3(vertices, a, xa);
            geom_load3(vertices, b, xb);
            geom_load3(vertices, c, xc);
            geom_load3(vertices, d, xd);
            // (4.3) the planarity guard, the corner roles fixed by the edge: n1 of (a, b, c), n2 of (b, a, d)
            dq_normal(xa, xb, xc, n1);
            dq_normal(xb, xa, xd, n2);
            const double dot = fl_dot(n1, n2);
            valid = dot >= 0.0 && dot * dot >= cos2 * (fl_dot(n1, n1) * fl_dot(n2, n2));
            // (4.4) neither new face, (a, d, c) and (b, c, d), turns over against the old pair
            if (valid) {
#pragma unroll
                for (int i = 0; i < 3; ++i) sum[i] = n1[i] + n2[i];
                dq_normal(xa, xd, xc, m1);
                dq_normal(xb, xc, xd, m2);
                valid = fl_dot(m1, sum) > 0.0 && fl_dot(m2, sum) > 0.0;
            }
            // (5) the worse quality of the pair must rise, strictly
            if (valid) {
                const double q_old = fl_min(fl_quality(a, xa, b, xb, c, xc), fl_quality(b, xb, a, xa, d, xd));
                const double q_new = fl_min(fl_quality(a, xa, d, xd, c, xc), fl_quality(b, xb, c, xc, d, xd));
                if (q_new > q_old)
                    k = (long long)(((unsigned long long)__float_as_uint((float)q_old) << 32) | (unsigned long long)((unsigned)e * FL_HASH));
            }
        }
    }
    const bool cand = k >= 0;
    key[e] = k;
    opp[4 * e] = cand ? c : 0;
    opp[4 * e + 1] = cand ? d : 0;
    opp[4 * e + 2] = cand ? f_ab : 0;
    opp[4 * e + 3] = cand ? f_ba : 0;
}

__global__ __launch_bounds__(FL_BLOCK) void fl_claim_init_kernel(long long* __restrict__ claim, long long n, long long* __restrict__ n_win) {
    const long v = (long)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (v < n) claim[v] = LLONG_MAX;
    if (v == 0) *n_win = 0;
}

__global__ __launch_bounds__(FL_BLOCK) void fl_claim_kernel(const int* __restrict__ edges, const long long* __restrict__ key,
                                                            const int* __restrict__ opp, const long long* __restrict__ n_edges,
                                                            long long max_edges, long long* __restrict__ claim) {
    const long e = (long)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (e >= max_edges || e >= *n_edges) return;
    const long long k = key[e];
    if (k < 0) return;
    atomicMin(claim + edges[2 * e], k);
    atomicMin(claim + edges[2 * e + 1], k);
    atomicMin(claim + opp[4 * e], k);
    atomicMin(claim + opp[4 * e + 1], k);
}

// FL_APPLY_EDGES edges per lane, a workgroup apart: a lane counts its winners, and the wave adds its sum to the counter once.
// One add per wave of 64 edges, 440 000 adds to the one address for 28 M edges, made the pass 5 ms where its loads and stores
// are a tenth of that.
constexpr int FL_APPLY_EDGES = 32;

__global__ __launch_bounds__(FL_BLOCK) void fl_apply_kernel(const int* __restrict__ edges, const long long* __restrict__ key,
                                                            const int* __restrict__ opp, const long long* __restrict__ n_edges,
                                                            long long max_edges, const long long* __restrict__ claim,
                                                            int* __restrict__ out_faces, unsigned char* __restrict__ win,
                                                            long long* __restrict__ n_win) {
    const long first = (long)blockIdx.x * (FL_BLOCK * FL_APPLY_EDGES) + threadIdx.x;
    const long long ne = *n_edges;
    int won = 0;
    for (int i = 0; i < FL_APPLY_EDGES; ++i) {
        const long e = first + (long)i * FL_BLOCK;
        if (e >= max_edges) break;
        bool w = false;
        const long long k = e < ne ? key[e] : -1;
        if (k >= 0) {
            const int a = edges[2 * e], b = edges[2 * e + 1], c = opp[4 * e], d = opp[4 * e + 1];
            w = claim[a] == k && claim[b] == k && claim[c] == k && claim[d] == k;
            if (w) {   // winners share no vertex, hence no face: plain stores
                const long f_ab = opp[4 * e + 2], f_ba = opp[4 * e + 3];
                out_faces[3 * f_ab] = a, out_faces[3 * f_ab + 1] = d, out_faces[3 * f_ab + 2] = c;
                out_faces[3 * f_ba] = b, out_faces[3 * f_ba + 1] = c, out_faces[3 * f_ba + 2] = d;
            }
        }
        win[e] = w ? 1 : 0;
        won += w ? 1 : 0;
    }
    // every lane of the wave is here again (the loop has no return): the sum over the wave, one add per wave with a winner
    won = wave_sum(won);
    if ((threadIdx.x & 63) == 0 && won != 0) atomicAdd((unsigned long long*)n_win, (unsigned long long)won);
}

}  // namespace d3d

using namespace d3d;

#define FL_CHECK_EDGES() D3D_REQUIRE(max_edges >= 0 && max_edges < (1ll << 31), "max_edges=%lld (0 .. 2^31 - 1)", max_edges)

extern "C" int d3d_mesh_flip_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                        const long long* offset, const int* nbr, const int* face_offset, const int* face_index,
                                        const int* edges, const long long* n_edges, long long max_edges, double cos2_max_angle,
                                        long long* key, int* opp, d3d_stream_t stream) {
    D3D_REQUIRE(vertices && faces && offset && nbr && face_offset && face_index && edges && n_edges && key && opp,
                "null pointer (vertices, faces, offset, nbr, face_offset, face_index, edges, n_edges, key, opp)");
    D3D_REQUIRE(dq_sizes_ok(n_vertices, n_faces), "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 6 n_faces < 2^31)", n_vertices,
                n_faces);
    FL_CHECK_EDGES();
    D3D_REQUIRE(cos2_max_angle >= 0.0 && cos2_max_angle < 1.0, "cos2_max_angle=%g must be in [0, 1): cos^2 of an angle in (0, 90] degrees",
                cos2_max_angle);
    if (max_edges == 0) return D3D_OK;
    hipLaunchKernelGGL(fl_candidates_kernel, dim3(ceil_div(max_edges, FL_BLOCK)), dim3(FL_BLOCK), 0, (hipStream_t)stream, vertices, faces, offset,
                       nbr, face_offset, face_index, edges, n_edges, max_edges, cos2_max_angle, key, opp);
    D3D_LAUNCH_CHECK("fl_candidates_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_flip_claim(long long n_vertices, const int* edges, const long long* key, const int* opp, const long long* n_edges,
                                   long long max_edges, long long* claim, long long* n_winners, d3d_stream_t stream) {
    D3D_REQUIRE(edges && key && opp && n_edges && claim && n_winners, "null pointer (edges, key, opp, n_edges, claim, n_winners)");
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    FL_CHECK_EDGES();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fl_claim_init_kernel, dim3(ceil_div(n_vertices > 0 ? n_vertices : 1, FL_BLOCK)), dim3(FL_BLOCK), 0, st, claim, n_vertices,
                       n_winners);
    D3D_LAUNCH_CHECK("fl_claim_init_kernel launch");
    if (max_edges == 0) return D3D_OK;
    hipLaunchKernelGGL(fl_claim_kernel, dim3(ceil_div(max_edges, FL_BLOCK)), dim3(FL_BLOCK), 0, st, edges, key, opp, n_edges, max_edges, claim);
    D3D_LAUNCH_CHECK("fl_claim_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_flip_apply(const int* faces, long long n_faces, const int* edges, const long long* key, const int* opp,
                                   const long long* n_edges, long long max_edges, const long long* claim, int* out_faces, unsigned char* win,
                                   long long* n_winners, d3d_stream_t stream) {
    D3D_REQUIRE((faces || n_faces == 0) && edges && key && opp && n_edges && claim && out_faces && win && n_winners,
                "null pointer (faces, edges, key, opp, n_edges, claim, out_faces, win, n_winners)");
    D3D_REQUIRE(dq_sizes_ok(0, n_faces), "n_faces=%lld (6 n_faces < 2^31)", n_faces);
    FL_CHECK_EDGES();
    D3D_REQUIRE(faces != out_faces, "faces and out_faces must be distinct buffers");
    hipStream_t st = (hipStream_t)stream;
    if (n_faces > 0) {
        const int rc = hip_status(hipMemcpyAsync(out_faces, faces, (size_t)n_faces * 12, hipMemcpyDeviceToDevice, st), "mesh flip apply: copy");
        if (rc != D3D_OK) return rc;
    }
    if (max_edges == 0) return D3D_OK;
    hipLaunchKernelGGL(fl_apply_kernel, dim3(ceil_div(max_edges, FL_BLOCK * FL_APPLY_EDGES)), dim3(FL_BLOCK), 0, st, edges, key, opp, n_edges,
                       max_edges, claim, out_faces, win, n_winners);
    D3D_LAUNCH_CHECK("fl_apply_kernel launch");
    return D3D_OK;
}
