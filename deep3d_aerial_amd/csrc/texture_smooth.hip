// Smoothing the texture's view choice over the mesh: the rule is this project's (deep3d_aerial_amd/texture.py
// states it, include/deep3d_planesweep.h too); it does not claim to match OpenMVS's TextureMesh.
//
// candidates: the selection's cull (tx_cull) and its per-view tests (tx_view_key), one workgroup per block of 256 faces.  Each
//             lane owns a face and keeps its TX_CANDIDATES smallest keys, sorted, in registers; a new key goes through a fully
//             unrolled compare-exchange chain (geom_list_insert), so no index into the list is a runtime value.
// merge:      one lane per face inserts the keys of one list into the other.
// smooth:     per round a propose and a commit launch, one lane per face.  Propose counts, per candidate, the weighted
//             neighbours of another id (a walk over the three corner rows of the vertex -> face CSR, one 4-byte gather of
//             cur_id per visit, the 16 ids and counts in registers), picks the cheapest admissible candidate and writes its
//             priority; commit lets a face change when its priority beats every neighbour's.  The host reads the commit
//             counts once per TS_READ rounds.
// Every value is written with ordinary vector stores; the one atomic is the integer add that counts a round's commits, whose
// return value is not used.  All float arithmetic is fp32 with IEEE-rounded operations and no contraction.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"
#include "texture_shared.h"

namespace d3d {

constexpr int TS_K = TX_CANDIDATES;
constexpr int TS_READ = 8;   // rounds between two reads of the commit counts

__device__ __forceinline__ void ts_load(const long long* __restrict__ cand, long f, long long (&c)[TS_K]) {
#pragma unroll
    for (int i = 0; i < TS_K; ++i) c[i] = cand[(long)TS_K * f + i];
}

__device__ __forceinline__ void ts_store(long long* __restrict__ cand, long f, const long long (&c)[TS_K]) {
#pragma unroll
    for (int i = 0; i < TS_K; ++i) cand[(long)TS_K * f + i] = c[i];
}

__global__ __launch_bounds__(TX_BLOCK) void ts_candidates_kernel(const float* __restrict__ vertices, long long n,
                                                                 const int* __restrict__ faces, long m,
                                                                 const d3d_ortho_view_t* __restrict__ views, int n_words, double tol1,
                                                                 const unsigned long long* __restrict__ mask, long long* __restrict__ cand) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    TxFrame T;
    const bool live = tx_frame(vertices, faces, f, m, n, &T);
    long long c[TS_K];
#pragma unroll
    for (int i = 0; i < TS_K; ++i) c[i] = TX_EMPTY;
    if (live) ts_load(cand, f, c);
    const unsigned long long* mk = mask + (long)blockIdx.x * n_words;
    for (int w = 0; w < n_words; ++w) {
        unsigned long long bits = mk[w];
        while (bits) {
            const int vi = __builtin_amdgcn_readfirstlane(w * 64 + __builtin_ctzll(bits));
            bits &= bits - 1;
            long long k;
            if (live && tx_view_key(views[vi], T, tol1, &k)) geom_list_insert(c, k, TX_EMPTY);
        }
    }
    if (live) ts_store(cand, f, c);
}

__global__ __launch_bounds__(TX_BLOCK) void ts_merge_kernel(const long long* a, const long long* b, long m, long long* out) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    long long c[TS_K], d[TS_K];
    ts_load(a, f, c);
    ts_load(b, f, d);
#pragma unroll
    for (int i = 0; i < TS_K; ++i) geom_list_insert(c, d[i], TX_EMPTY);
    ts_store(out, f, c);   // after both rows are read: out may be a or b
}

// ---------------------------------------------------------------------------------------------------------------------------
// smoothing
// ---------------------------------------------------------------------------------------------------------------------------
// label 0 and the first candidate's id for a face of three distinct indices with a candidate; -1 and -1 otherwise.
__global__ __launch_bounds__(TX_BLOCK) void ts_init_kernel(const long long* __restrict__ cand, const int* __restrict__ faces, long m,
                                                           long long n, int* __restrict__ label, int* __restrict__ cur_id) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    int a, b, c;
    const long long k0 = cand[(long)TS_K * f];
    const bool has = geom_face<true>(faces, f, n, &a, &b, &c) && k0 != TX_EMPTY;
    label[f] = has ? 0 : -1;
    cur_id[f] = has ? geom_key_id(k0) : -1;
}

// The rows of face f's corners in the vertex -> face CSR, clipped to the arrays: visit(g) for every entry g != f in 0 .. m - 1.
template <typename Visit>
__device__ __forceinline__ void ts_walk(long f, long m, int a, int b, int c, const int* __restrict__ face_offset,
                                        const int* __restrict__ face_index, Visit visit) {
    const int idx[3] = {a, b, c};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const long s = max(face_offset[idx[q]], 0), e = min((long)face_offset[idx[q] + 1], 3 * m);
        for (long j = s; j < e; ++j) {
            const int g = face_index[j];
            if (g != (int)f && (unsigned)g < (unsigned long)m) visit(g);
        }
    }
}

__global__ __launch_bounds__(TX_BLOCK) void ts_propose_kernel(const long long* __restrict__ cand, const int* __restrict__ faces, long m,
                                                              long long n, const int* __restrict__ face_offset,
                                                              const int* __restrict__ face_index, const int* __restrict__ label,
                                                              const int* __restrict__ cur_id, float weight, float max_loss,
                                                              long long* __restrict__ prio, int* __restrict__ prop) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    const int l = label[f];
    int a, b, c;
    if (l < 0 || l >= TS_K || !geom_face<true>(faces, f, n, &a, &b, &c)) {
        prio[f] = 0;
        return;
    }
    long long key[TS_K];
    ts_load(cand, f, key);
    int id[TS_K], cnt[TS_K];
#pragma unroll
    for (int k = 0; k < TS_K; ++k) {
        id[k] = geom_key_id(key[k]);
        cnt[k] = 0;
    }
    ts_walk(f, m, a, b, c, face_offset, face_index, [&](int g) {
        const int ig = cur_id[g];
        if (ig < 0) return;   // no winner: walked over, not counted
#pragma unroll
        for (int k = 0; k < TS_K; ++k) cnt[k] += ig != id[k] ? 1 : 0;
    });
    const float s0 = __uint_as_float((unsigned)(key[0] >> 32));
    float c_cur = 0.0f, c_best = INFINITY;
    int best = -1;
#pragma unroll
    for (int k = 0; k < TS_K; ++k) {
        const float d = __fsub_rn(1.0f, __fdiv_rn(s0, __uint_as_float((unsigned)(key[k] >> 32))));
        const float ck = __fadd_rn(d, __fmul_rn(weight, (float)cnt[k]));
        const bool ok = k == 0 || (key[k] != TX_EMPTY && d <= max_loss);
        c_cur = k == l ? ck : c_cur;
        if (ok && ck < c_best) {
            c_best = ck;
            best = k;
        }
    }
    const float gain = __fsub_rn(c_cur, c_best);
    if (best >= 0 && gain > 0.0f) {
        prio[f] = ((long long)__float_as_uint(gain) << 32) | (long long)(0xffffffffu - (unsigned)f);
        prop[f] = best;
    } else {
        prio[f] = 0;
    }
}

__global__ __launch_bounds__(TX_BLOCK) void ts_commit_kernel(const long long* __restrict__ cand, const int* __restrict__ faces, long m,
                                                             long long n, const int* __restrict__ face_offset,
                                                             const int* __restrict__ face_index, const long long* __restrict__ prio,
                                                             const int* __restrict__ prop, int* __restrict__ label,
                                                             int* __restrict__ cur_id, int* __restrict__ commits) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    bool take = false;
    if (f < m) {
        const long long p = prio[f];
        int a, b, c;
        if (p > 0 && geom_face<true>(faces, f, n, &a, &b, &c)) {
            take = true;
            ts_walk(f, m, a, b, c, face_offset, face_index, [&](int g) { take = take && p > prio[g]; });
        }
        if (take) {
            const int l = min(max(prop[f], 0), TS_K - 1);
            label[f] = l;
            cur_id[f] = geom_key_id(cand[(long)TS_K * f + l]);
        }
    }
    const unsigned long long won = __ballot(take);
    if (won && (threadIdx.x & 63) == __builtin_ctzll(won)) atomicAdd(commits, __builtin_popcountll(won));
}

__global__ __launch_bounds__(TX_BLOCK) void ts_keys_kernel(const long long* __restrict__ cand, const int* __restrict__ label, long m,
                                                           long long* __restrict__ key_out) {
    const long f = (long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (f >= m) return;
    const int l = label[f];
    key_out[f] = l >= 0 && l < TS_K ? cand[(long)TS_K * f + l] : TX_EMPTY;
}

struct TsScratch {
    size_t cur_id, prio, prop, bytes;
};

static TsScratch ts_layout(long long m) {
    const size_t nf = (size_t)(m > 0 ? m : 1);
    ScratchLayout L;
    TsScratch s;
    s.cur_id = L.take(nf * 4);
    s.prio = L.take(nf * 8);
    s.prop = L.take(nf * 4);
    s.bytes = L.bytes;
    return s;
}

// d3d_mesh_decimate_incidence's limit: the CSR's offsets are int32
static bool ts_sizes_ok(long long n, long long m) { return n >= 0 && n < (1ll << 31) && m >= 0 && 6 * m < (1ll << 31); }

}  // namespace d3d

using namespace d3d;

extern "C" int d3d_texture_candidates_max(void) { return TX_CANDIDATES; }

extern "C" int d3d_texture_candidates(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                      const d3d_ortho_view_t* views, int n_views, double depth_tolerance, void* scratch,
                                      size_t scratch_bytes, long long* cand, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && (faces || n_faces == 0) && (cand || n_faces == 0), "null pointer (vertices, faces, cand)");
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31) && n_faces >= 0 && 3 * n_faces < (1ll << 31),
                "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 3 n_faces < 2^31)", n_vertices, n_faces);
    D3D_REQUIRE(n_views >= 0 && n_views < (1 << 20), "%d views (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    D3D_REQUIRE(std::isfinite(depth_tolerance) && depth_tolerance >= 0.0, "depth_tolerance=%g must be finite and >= 0", depth_tolerance);
    if (n_views == 0 || n_faces == 0) return D3D_OK;
    const size_t need = tx_mask_bytes(n_faces, n_views);
    D3D_REQUIRE(scratch, "null pointer (scratch)");
    D3D_REQUIRE(scratch_bytes >= need, "scratch of %zu bytes, %zu needed (d3d_texture_scratch_bytes)", scratch_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* mask = (unsigned long long*)scratch;
    const int rc = tx_cull(vertices, n_vertices, faces, n_faces, views, n_views, mask, st);
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(ts_candidates_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, st, vertices, n_vertices, faces,
                       (long)n_faces, views, ceil_div(n_views, 64), 1.0 + depth_tolerance, mask, cand);
    D3D_LAUNCH_CHECK("ts_candidates_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_texture_candidates_merge(const long long* a, const long long* b, long long n_faces, long long* out, d3d_stream_t stream) {
    D3D_REQUIRE((a && b && out) || n_faces == 0, "null pointer (a, b, out)");
    D3D_REQUIRE(n_faces >= 0 && 3 * n_faces < (1ll << 31), "n_faces=%lld (3 n_faces < 2^31)", n_faces);
    if (n_faces == 0) return D3D_OK;
    hipLaunchKernelGGL(ts_merge_kernel, dim3(ceil_div(n_faces, TX_BLOCK)), dim3(TX_BLOCK), 0, (hipStream_t)stream, a, b, (long)n_faces, out);
    D3D_LAUNCH_CHECK("ts_merge_kernel launch");
    return D3D_OK;
}

extern "C" size_t d3d_texture_smooth_scratch_bytes(long long n_faces) {
    if (!ts_sizes_ok(0, n_faces)) return 0;
    return ts_layout(n_faces).bytes;
}

extern "C" int d3d_texture_smooth(const long long* cand, long long n_faces, const int* faces, long long n_vertices, const int* face_offset,
                                  const int* face_index, float weight, float max_loss, int rounds, void* scratch, size_t scratch_bytes,
                                  int* label, long long* key_out, int* commits, int* rounds_run, d3d_stream_t stream) {
    D3D_REQUIRE(((cand && faces && label && key_out) || n_faces == 0) && face_offset && (face_index || n_faces == 0) && commits && scratch,
                "null pointer (cand, faces, face_offset, face_index, label, key_out, commits, scratch)");
    D3D_REQUIRE(ts_sizes_ok(n_vertices, n_faces),
                "n_vertices=%lld, n_faces=%lld: the smoothing walks d3d_mesh_decimate_incidence's rows (0 .. 2^31 - 1 vertices, 6 n_faces < 2^31)",
                n_vertices, n_faces);
    D3D_REQUIRE(std::isfinite(weight) && weight > 0.0f, "weight=%g must be finite and > 0", (double)weight);
    D3D_REQUIRE(max_loss >= 0.0f && max_loss <= 1.0f, "max_loss=%g must lie in [0, 1]", (double)max_loss);
    D3D_REQUIRE(rounds >= 1 && rounds <= 1024, "rounds=%d (1 .. 1024)", rounds);
    const TsScratch L = ts_layout(n_faces);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed (d3d_texture_smooth_scratch_bytes)", scratch_bytes, L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    int *cur_id = (int*)(w + L.cur_id), *prop = (int*)(w + L.prop);
    long long* prio = (long long*)(w + L.prio);
    const long m = (long)n_faces;
    int rc = hip_status(hipMemsetAsync(commits, 0, (size_t)rounds * 4, st), "texture smooth: clear commits");
    if (rc != D3D_OK) return rc;
    if (rounds_run) *rounds_run = 0;
    if (m == 0) return D3D_OK;
    const dim3 grid(ceil_div(m, TX_BLOCK)), block(TX_BLOCK);
    hipLaunchKernelGGL(ts_init_kernel, grid, block, 0, st, cand, faces, m, n_vertices, label, cur_id);
    D3D_LAUNCH_CHECK("ts_init_kernel launch");
    int r = 0, run = rounds;
    bool fixed = false;
    while (r < rounds && !fixed) {
        const int r0 = r, nb = rounds - r < TS_READ ? rounds - r : TS_READ;
        for (; r < r0 + nb; ++r) {
            hipLaunchKernelGGL(ts_propose_kernel, grid, block, 0, st, cand, faces, m, n_vertices, face_offset, face_index, label, cur_id,
                               weight, max_loss, prio, prop);
            D3D_LAUNCH_CHECK("ts_propose_kernel launch");
            hipLaunchKernelGGL(ts_commit_kernel, grid, block, 0, st, cand, faces, m, n_vertices, face_offset, face_index, prio, prop, label,
                               cur_id, commits + r);
            D3D_LAUNCH_CHECK("ts_commit_kernel launch");
        }
        int host[TS_READ];
        rc = hip_status(hipMemcpyAsync(host, commits + r0, (size_t)nb * 4, hipMemcpyDeviceToHost, st), "texture smooth: read commits");
        if (rc != D3D_OK) return rc;
        rc = hip_status(hipStreamSynchronize(st), "texture smooth: sync");
        if (rc != D3D_OK) return rc;
        for (int i = 0; i < nb && !fixed; ++i)
            if (host[i] == 0) {
                fixed = true;
                run = r0 + i + 1;   // rounds after it changed nothing
            }
    }
    if (rounds_run) *rounds_run = run;
    hipLaunchKernelGGL(ts_keys_kernel, grid, block, 0, st, cand, label, m, key_out);
    D3D_LAUNCH_CHECK("ts_keys_kernel launch");
    return D3D_OK;
}
