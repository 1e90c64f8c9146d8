// Rejecting photo-inconsistent views from the texture's candidate lists: the rule is this project's
// (deep3d_aerial_amd/texture.py states it, include/deep3d_planesweep.h too); it does not claim to match OpenMVS's TextureMesh.
//
// colours:  one lane per face, looping over the slots of its candidate list.  The lanes of a wave hold neighbouring faces, whose
//           lists mostly name the same views, so the 16 four-byte gathers of a slot (four bilinear taps, geom_tap) fall into the
//           same image; the 128-byte cand rows and 64-byte col rows are strided across the wave instead.  The view is found by
//           bisection (tx_find), the corners are projected per view (tx_corner_uv).
//           The word of a slot depends on its face, key and view alone, so batches and ranks fill disjoint slots of one col.
//           Built with -DD3D_COLORS_PER_SLOT the pass is one lane per (face, slot) instead, which coalesces the rows and
//           scatters the gathers: the build tools/texture_bench.py --variant_library times beside this one.
// outliers: one lane per face.  The 16 keys and the 16 colour words sit in registers; the per-channel lower median is found by
//           rank counting, fully unrolled, so no index into a register array is a runtime value; the surviving keys are
//           written at a running index in global memory after every key of the row has been read, so cand_out may be cand.
// Every value is written with ordinary vector stores; the one atomic is the integer add of a wave's share of the four counters,
// whose return value is not used.  The colours are fp64 with no contraction, the vote is all integer.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"
#include "texture_shared.h"

namespace d3d {

constexpr int TO_K = TX_CANDIDATES;
constexpr int TO_QMAX = 1020;   // four times 255: a channel in quarter grey levels

// The colour word of face F in view V (texture.py "Colour of a face in a candidate view"): false when a corner does not project.
__device__ __forceinline__ bool to_word(const d3d_ortho_view_t& V, const TxFace& F, int* word_out) {
    double u[3], v[3];
    if (!tx_corner_uv(V, F, u, v)) return false;
    // the centroid, then each corner weighted 4 : 1 : 1, every sum left to right
    const double su[4] = {((u[0] + u[1]) + u[2]) / 3.0, ((4.0 * u[0] + u[1]) + u[2]) / 6.0, ((4.0 * u[1] + u[0]) + u[2]) / 6.0,
                          ((4.0 * u[2] + u[0]) + u[1]) / 6.0};
    const double sv[4] = {((v[0] + v[1]) + v[2]) / 3.0, ((4.0 * v[0] + v[1]) + v[2]) / 6.0, ((4.0 * v[1] + v[0]) + v[2]) / 6.0,
                          ((4.0 * v[2] + v[0]) + v[1]) / 6.0};
    double t[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s) geom_tap(V.rgba, V.W, V.H, su[s], sv[s], t[s]);
    unsigned word = 1u << 30;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double q = fmin(fmax(floor((((t[0][ch] + t[1][ch]) + t[2][ch]) + t[3][ch]) + 0.5), 0.0), (double)TO_QMAX);
        word |= (unsigned)q << (20 - 10 * ch);
    }
    *word_out = (int)word;
    return true;
}

// The view of a key in the call's table when it has an image, else null.
__device__ __forceinline__ const d3d_ortho_view_t* to_view(const d3d_ortho_view_t* __restrict__ views, int n_views, long long key) {
    if (key == TX_EMPTY) return nullptr;
    const int vi = tx_find(views, n_views, geom_key_id(key));
    if (vi < 0) return nullptr;
    const d3d_ortho_view_t* V = views + vi;
    return V->rgba && V->W >= 1 && V->H >= 1 ? V : nullptr;
}

#ifndef D3D_COLORS_PER_SLOT
constexpr int TO_LANES_PER_FACE = 1;
__global__ __launch_bounds__(TX_BLOCK) void to_colors_kernel(const float* __restrict__ vertices, long long n,
                                                             const int* __restrict__ faces, long m,
                                                             const long long* __restrict__ cand,
                                                             const d3d_ortho_view_t* __restrict__ views, int n_views,
                                                             int* __restrict__ col) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    TxFace F;
    if (!tx_face(vertices, faces, f, n, &F)) return;
#pragma unroll 1
    for (int k = 0; k < TO_K; ++k) {
        const long i = (long)TO_K * f + k;
        const d3d_ortho_view_t* V = to_view(views, n_views, cand[i]);
        int word;
        if (V && to_word(*V, F, &word)) col[i] = word;
    }
}
#else
constexpr int TO_LANES_PER_FACE = TO_K;
__global__ __launch_bounds__(TX_BLOCK) void to_colors_kernel(const float* __restrict__ vertices, long long n,
                                                             const int* __restrict__ faces, long m,
                                                             const long long* __restrict__ cand,
                                                             const d3d_ortho_view_t* __restrict__ views, int n_views,
                                                             int* __restrict__ col) {
    const long i = (long)blockIdx.x * TX_BLOCK + threadIdx.x;   // slot i & 15 of face i >> 4
    if (i >= (long)TO_K * m) return;
    const d3d_ortho_view_t* V = to_view(views, n_views, cand[i]);
    if (!V) return;
    TxFace F;
    int word;
    if (tx_face(vertices, faces, i / TO_K, n, &F) && to_word(*V, F, &word)) col[i] = word;
}
#endif

__global__ __launch_bounds__(TX_BLOCK) void to_vote_kernel(const long long* cand, const int* __restrict__ col, long m, int T,
                                                           long long* cand_out, int* __restrict__ rejected, int* __restrict__ counts) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    const bool live = f < m;
    int tested = 0, changed = 0, removed = 0, kept_all = 0;
    if (live) {
        long long key[TO_K];
        int w[TO_K];
#pragma unroll
        for (int k = 0; k < TO_K; ++k) key[k] = cand[(long)TO_K * f + k];
        const int4* row = (const int4*)(col + (long)TO_K * f);
#pragma unroll
        for (int k = 0; k < TO_K; k += 4) {
            const int4 c = row[k >> 2];
            w[k] = c.x, w[k + 1] = c.y, w[k + 2] = c.z, w[k + 3] = c.w;
        }
        bool valid[TO_K];
        int n_valid = 0;
#pragma unroll
        for (int k = 0; k < TO_K; ++k) {
            valid[k] = key[k] != TX_EMPTY && w[k] != 0;
            n_valid += valid[k] ? 1 : 0;
        }
        unsigned out_mask = 0;   // bit k: slot k is removed
        if (n_valid >= 3) {
            tested = 1;
            const int target = (n_valid - 1) >> 1;
            int dev[TO_K];
#pragma unroll
            for (int k = 0; k < TO_K; ++k) dev[k] = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                // (q << 4) | k orders the valid values by (q, slot); an invalid slot is above them all
                int s[TO_K];
#pragma unroll
                for (int k = 0; k < TO_K; ++k) s[k] = valid[k] ? (((w[k] >> (20 - 10 * ch)) & 1023) << 4) | k : INT_MAX;
                int med = 0;
#pragma unroll
                for (int k = 0; k < TO_K; ++k) {
                    int rank = 0;
#pragma unroll
                    for (int j = 0; j < TO_K; ++j) rank += s[j] < s[k] ? 1 : 0;
                    med = valid[k] && rank == target ? s[k] >> 4 : med;
                }
#pragma unroll
                for (int k = 0; k < TO_K; ++k) dev[k] = max(dev[k], abs((s[k] >> 4) - med));
            }
            int n_out = 0;
#pragma unroll
            for (int k = 0; k < TO_K; ++k) {
                const bool out = valid[k] && dev[k] > T;
                out_mask |= out ? 1u << k : 0u;
                n_out += out ? 1 : 0;
            }
            if (n_out == n_valid) {   // the three medians may belong to three views: the face keeps its list
                kept_all = 1;
                out_mask = 0;
                n_out = 0;
            }
            removed = n_out;
        }
        // every key of the row is in registers by now, so cand_out may be cand
        long long* dst = cand_out + (long)TO_K * f;
        int at = 0;
        long long first = TX_EMPTY;
#pragma unroll
        for (int k = 0; k < TO_K; ++k) {
            if (key[k] != TX_EMPTY && !((out_mask >> k) & 1u)) {
                first = at == 0 ? key[k] : first;
                dst[at++] = key[k];
            }
        }
        for (; at < TO_K; ++at) dst[at] = TX_EMPTY;
        changed = first != key[0] ? 1 : 0;
        rejected[f] = (int)out_mask;
    }
    wave_counts_add(counts, tested, changed, removed, kept_all);
}

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_texture_face_colors(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                       const long long* cand, const d3d_ortho_view_t* views, int n_views, int* col, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && ((faces && cand && col) || n_faces == 0), "null pointer (vertices, faces, cand, col)");
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31) && n_faces >= 0 && 3 * n_faces < (1ll << 31),
                "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 3 n_faces < 2^31)", n_vertices, n_faces);
    D3D_REQUIRE(n_views >= 0 && n_views < (1 << 20), "%d views (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    if (n_views == 0 || n_faces == 0) return D3D_OK;
    hipLaunchKernelGGL(to_colors_kernel, dim3(ceil_div((long)TO_LANES_PER_FACE * n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream,
                       vertices, n_vertices, faces, (long)n_faces, cand, views, n_views, col);
    D3D_LAUNCH_CHECK("to_colors_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_outliers(const long long* cand, const int* col, long long n_faces, int T, long long* cand_out, int* rejected,
                                    int* counts, d3d_stream_t stream) {
    D3D_REQUIRE(((cand && col && cand_out && rejected) || n_faces == 0) && counts, "null pointer (cand, col, cand_out, rejected, counts)");
    D3D_REQUIRE(n_faces >= 0 && 3 * n_faces < (1ll << 31), "n_faces=%lld (3 n_faces < 2^31)", n_faces);
    D3D_REQUIRE(T >= 0 && T <= TO_QMAX, "T=%d (0 .. %d quarter grey levels)", T, TO_QMAX);
    hipStream_t st = (hipStream_t)stream;
    const int rc = hip_status(hipMemsetAsync(counts, 0, 4 * sizeof(int), st), "texture outliers: clear counts");
    if (rc != D3D_OK) return rc;
    if (n_faces == 0) return D3D_OK;
    hipLaunchKernelGGL(to_vote_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, st, cand, col, (long)n_faces, T, cand_out,
                       rejected, counts);
    D3D_LAUNCH_CHECK("to_vote_kernel launch");
    return D3D_OK;
}
